"""Time make_ccf.build_ccf_set on an arm of DESI size: every 7th template of a 7^4
synthetic grid at three vsini values (1029 model rows) on a template grid of ~6400
pixels, N_fft 8192.

    python tools/perf/ccf_set_timing.py [--reps 5]
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/perf/ccf_set_timing.py --reps 2

Prints one JSON line: HIP-event times (ms, median of the repetitions after one warm-up
call) of the whole build_ccf_set call -- selection and tables on the host, uploads, the
launches, the copy of the set back to the host -- and of its device part alone
(rvs_ccf_model_rows + rvs_vsini_convolve + rvs_ccf_models_build).  The kernels' share
comes from the rocprofv3 run (ccf_model_kernel, ccf_rfft_kernel<true>)."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(
    os.path.abspath(__file__)))))
from rvspecfit_amd import make_ccf, synth          # noqa: E402
from rvspecfit_amd.library import TemplateLibrary   # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    a = ap.parse_args()
    l0, l1, step = 3600., 5800., 0.37
    lib = synth.make_interp_library_fast('timing_b', l0 - 40, l1 + 40, step,
                                         resol=3000., device='cuda')
    tl = TemplateLibrary('timing_b', synth.library_as_npz_dict(lib, None))
    cc = make_ccf.get_ccf_config(np.log(l0), np.log(l1), 8192)
    vs = [0., 100., 300.]
    inner = []
    real = make_ccf.models_build

    def timed(*args, **kw):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        r = real(*args, **kw)
        e1.record()
        inner.append((e0, e1))
        return r
    make_ccf.models_build = timed
    whole = []
    s = None
    for rep in range(a.reps + 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        s = make_ccf.build_ccf_set(tl, cc, every=7, vsinis=vs)
        e1.record()
        torch.cuda.synchronize()
        whole.append(e0.elapsed_time(e1))
    inner_ms = [x.elapsed_time(y) for x, y in inner]
    print(json.dumps(dict(rows=int(s['ccf_mod'].shape[0]), ntp=int(tl.ntp), nfft=8192,
                          nnode=make_ccf.model_tables(tl.lam, cc)['nnode'],
                          first_call_ms=round(whole[0], 2),
                          build_ccf_set_ms=round(float(np.median(whole[1:])), 2),
                          models_build_ms=round(float(np.median(inner_ms[1:])), 2),
                          all_ms=[round(w, 2) for w in whole[1:]])))


if __name__ == '__main__':
    main()
