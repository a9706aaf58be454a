#!/opt/conda/bin/python3.9
"""Golden vectors for the options of rvs_make_interpol that the committed libraries
(lib_gold_*, lib_desi_*, lib_sdss1: --resol 2000, vacuum, log step, linear_continuum,
float32) do not exercise: --air, --resol_func, --fixed_fwhm, --normalize median / none,
--no-log, --float_bits 64.

    bash tests/golden/setup_reference_scratch.sh
    /opt/conda/bin/python3.9 -W ignore tests/golden/make_golden_interpol.py

IMPORTS the reference (build container only).  The high-resolution models are written
by the build's own generator (rvspecfit_amd.synth) on a 2^4 grid and a short range; the
reference's read_grid -> make_interpol -> make_nd --regulargrid run on them once per
case.  Written: interpol_cases.npz -- the recipe of the inputs (grid, wavelengths, the
options of each case) and the reference's outputs (lam, dats, vec, idgrid, uvec*,
lognorms, log_step per case).  Data only.
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
sys.modules['numba'] = None
sys.modules['numdifftools'] = types.ModuleType('numdifftools')

import numpy as np  # noqa: E402
from rvspecfit import read_grid, make_interpol, make_nd, serializer  # noqa: E402
from rvspecfit_amd import synth  # noqa: E402

WORK = '/tmp/golden_work_interpol'
GRID_KW = dict(nteff=2, nlogg=2, nfeh=2, nalpha=2, teff_range=(4500., 6500.),
               logg_range=(2., 4.), feh_range=(-1., 0.), alpha_range=(0., 0.4))
LAM_HR = (4450., 4650., 10001)          # np.linspace
RANGE = ('--lambda0', '4500', '--lambda1', '4600', '--step', '0.4')
CASES = {
    'air': ('--resol', '2000', '--air'),
    'resol_func': ('--resol_func', '1500+0.1*x'),
    'fixed_fwhm': ('--resol', '2000', '--fixed_fwhm'),
    'median': ('--resol', '2000', '--normalize', 'median'),
    'none': ('--resol', '2000', '--normalize', 'none'),
    'nolog': ('--resol', '2000', '--no-log'),
    'f64': ('--resol', '2000', '--float_bits', '64'),
    # the photon factor uses the wavelengths as given, the rebinner the air ones: a
    # median normalisation keeps the difference (a linear continuum divides it out)
    'air_median_f64': ('--resol', '2000', '--air', '--normalize', 'median',
                       '--float_bits', '64'),
}


def main():
    if os.path.exists(WORK):
        shutil.rmtree(WORK)
    pref = WORK + '/hr/'
    os.makedirs(pref)
    synth.write_fits_grid(pref, 'wave.fits', grid_kw=GRID_KW,
                          lam_hr=np.linspace(*LAM_HR))
    db = WORK + '/files.db'
    read_grid.main(['--prefix', pref, '--templdb', db])
    out = {'lam_hr': np.array(LAM_HR), 'cases': np.array(list(CASES))}
    for k, v in GRID_KW.items():
        out['grid/' + k] = np.asarray(v, dtype=np.float64)
    for name, opts in CASES.items():
        templ = WORK + '/templ_%s/' % name
        os.makedirs(templ)
        args = list(RANGE) + list(opts)
        make_interpol.main(['--templdb', db, '--wavefile', pref + 'wave.fits',
                            '--templprefix', pref, '--setup', name, '--oprefix', templ,
                            '--nthreads', '1'] + args)
        make_nd.main(['--setup', name, '--prefix', templ, '--regulargrid'])
        fd = serializer.load_dict_from_hdf5(templ + make_nd.INTERPOL_H5_NAME % name)
        dats = np.load(templ + make_nd.INTERPOL_DAT_NAME % name)
        out[name + '/args'] = np.array(args)
        out[name + '/lam'] = np.asarray(fd['lam'])
        out[name + '/dats'] = dats
        out[name + '/vec'] = np.asarray(fd['vec'])
        out[name + '/idgrid'] = np.asarray(fd['idgrid'])
        out[name + '/lognorms'] = np.asarray(fd['lognorms'])
        out[name + '/log_step'] = np.array(bool(fd['log_step']))
        for i, u in enumerate(fd['uvecs']):
            out[name + '/uvec%d' % i] = np.asarray(u)
        print(name, dats.dtype, dats.shape)
    np.savez_compressed(HERE + '/interpol_cases.npz', **out)


if __name__ == '__main__':
    main()
