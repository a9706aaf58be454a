#!/opt/conda/bin/python3.9
"""The HDF5 files of the setup gold_b as the reference's prep pipeline writes them:
input of tools/convert_artefacts.py in
tests/test_tools_cpu.py::test_convert_artefacts_reproduces_reference_loader.

    bash tests/golden/setup_reference_scratch.sh
    /opt/conda/bin/python3.9 -W ignore tests/golden/make_golden_convert.py

IMPORTS the reference (build container only).  The artefacts are those of
make_golden.py and make_golden_nocont.py, written once more by the reference's own
make_nd / make_ccf.  Kept, under tests/golden/templ_gold_b/ (data only):
  interp_gold_b.h5  ccf_gold_b.h5  ccf_nocont_gold_b.h5
What the reference's loader (serializer.load_dict_from_hdf5) returns for them must be
what lib_gold_b.npz / lib_nocont_gold_b.npz hold, bit for bit: checked here.  The
array files next to them (interpdat_*.npy, ccfdat_*.npz, ccfmod_*.npy) are not kept:
the test writes them from the same two fixtures (an FFT of another numpy build
differs from the stored CCF arrays in the last bit).
"""
import os
import shutil
import sys
import types

os.environ['OMP_NUM_THREADS'] = '1'
HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.abspath(HERE + '/../..')
sys.path.insert(0, '/tmp/oracle')
sys.path.insert(0, REPO)
sys.path.insert(0, HERE)
sys.modules['numba'] = None
sys.modules['numdifftools'] = types.ModuleType('numdifftools')

import numpy as np  # noqa: E402
import make_golden as MG  # noqa: E402  (imports the reference)
from rvspecfit import make_ccf, make_nd, serializer  # noqa: E402

NAME = 'gold_b'
OUT = HERE + '/templ_' + NAME


def ccf_keys(pref, continuum):
    ci = serializer.load_dict_from_hdf5(
        MG.TEMPL + make_ccf.get_ccf_info_name(NAME, continuum))
    cc = ci['ccfconf']
    vs = np.array([np.nan if _ is None else _ for _ in ci['vsinis']], dtype=float)
    out = {pref + 'params': np.asarray(ci['params'], dtype=float),
           pref + 'vsinis': vs,
           pref + 'parnames': np.array(list(ci['parnames'])),
           pref + 'logl0': np.array(cc['logl0']),
           pref + 'logl1': np.array(cc['logl1']),
           pref + 'npoints': np.array(cc['npoints']),
           pref + 'continuum': np.array(bool(cc['continuum'])),
           pref + 'maxcontpts': np.array(cc['maxcontpts'])}
    if continuum:
        out[pref + 'splinestep'] = np.array(cc['splinestep'])
    return out


def main():
    MG.build_reference_artefacts()
    c0, c1, cs = MG.SETUPS[NAME]['ccf']
    make_ccf.main([
        '--setup', NAME, '--prefix', MG.TEMPL, '--lambda0', str(c0), '--lambda1',
        str(c1), '--step', str(cs), '--every', '20', '--vsinis', '0,100',
        '--oprefix', MG.TEMPL, '--nthreads', '1', '--nocontinuum'])
    # (the HDF5-borne keys of make_golden.export_library / make_golden_nocont)
    fd = serializer.load_dict_from_hdf5(MG.TEMPL + make_nd.INTERPOL_H5_NAME % NAME)
    out = dict(
        lam=fd['lam'], vec=fd['vec'], idgrid=fd['idgrid'],
        log_step=np.array(bool(fd['log_step'])),
        log_ids=np.array(fd['mapper_args'][0], dtype=np.int64),
        parnames=np.array(list(fd['parnames'])))
    for i, u in enumerate(fd['uvecs']):
        out['uvec%d' % i] = np.asarray(u)
    out.update(ccf_keys('ccf_', True))
    out.update(ccf_keys('ccfnc_', False))
    gold = dict(np.load(HERE + '/lib_%s.npz' % NAME))
    gold.update(np.load(HERE + '/lib_nocont_%s.npz' % NAME))
    arrays = {p + k for p in ('ccf_', 'ccfnc_') for k in ('fft', 'fft2', 'mod')}
    assert set(out) == set(gold) - arrays - {'dats'}
    for k, v in out.items():
        assert np.asarray(v).shape == gold[k].shape and \
            np.array_equal(v, gold[k], equal_nan=np.asarray(v).dtype.kind == 'f'), k
    if os.path.exists(OUT):
        shutil.rmtree(OUT)
    os.makedirs(OUT)
    for f in sorted(os.listdir(MG.TEMPL)):
        if NAME in f and f.endswith('.h5') and not f.startswith('specs_'):
            shutil.copy(MG.TEMPL + f, OUT)
    print('wrote', sorted(os.listdir(OUT)))


if __name__ == '__main__':
    main()
