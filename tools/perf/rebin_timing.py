"""Time the three kernels behind make_interpol.build_specs on an arm of DESI size from
input at PHOENIX spacing: synth.DESI_ARMS['b'] (6215 output pixels) from 0.006 A input
(~410 000 pixels), R = 2000, 10 000 synthetic models generated on the device in chunks
as float32.

    python tools/perf/rebin_timing.py [--templates 10000] [--chunk 250] [--host 1000]

Prints one JSON line: HIP-event times (ms) of the band build (rvs_rebin_weights, median
of three calls after a warm-up), of rvs_rebin_apply and rvs_template_normalize summed
over the chunks (one warm-up chunk first), the multiply-adds of the apply and its rate,
and -- for --host models held in host memory -- the time of the same work including
the copy to the device, i.e. the transfer's share."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(
    os.path.abspath(__file__)))))
from rvspecfit_amd import make_interpol, read_grid, synth   # noqa: E402


def ev():
    return torch.cuda.Event(enable_timing=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--templates', type=int, default=10000)
    ap.add_argument('--chunk', type=int, default=250)
    ap.add_argument('--host', type=int, default=1000)
    ap.add_argument('--hr-step', type=float, default=0.006)
    a = ap.parse_args()
    l0, l1, step = synth.DESI_ARMS['b']['templ']
    lam = make_interpol.output_grid(l0, l1, step, True)
    lam_hr = np.arange(l0 * 0.99, l1 * 1.01, a.hr_step)
    R = make_interpol.Resolution(resol=2000.)
    band = []
    for rep in range(4):
        e0, e1 = ev(), ev()
        e0.record()
        mat = read_grid.make_rebinner(lam_hr, lam, R, resolution0=100000, toair=False)
        e1.record()
        torch.cuda.synchronize()
        band.append(e0.elapsed_time(e1))
    nwin = (mat.right - mat.left + 2).sum().item()
    rng = np.random.default_rng(1)
    t_apply, t_norm = [], []
    out = torch.empty((a.chunk, len(lam)), dtype=torch.float32, device='cuda')
    done = -a.chunk                    # the first chunk is the warm-up
    while done < a.templates:
        n = a.chunk
        p = [torch.as_tensor(rng.uniform(lo, hi, size=n)).to('cuda')
             for lo, hi in ((3500., 7500.), (1., 4.), (-2., 0.), (0., 0.4))]
        hr = synth.spectra_batch(lam_hr, *p, xp=torch).float()[:, mat.col0:mat.col1]
        hr = hr.contiguous()
        e0, e1, e2 = ev(), ev(), ev()
        e0.record()
        rows = read_grid.apply_band(mat, hr, True)
        e1.record()
        make_interpol.normalize_rows(rows, lam, 'linear_continuum', True, 32, out=out)
        e2.record()
        torch.cuda.synchronize()
        if done >= 0:
            t_apply.append(e0.elapsed_time(e1))
            t_norm.append(e1.elapsed_time(e2))
        done += n
    T = len(t_apply) * a.chunk
    res = dict(templates=T, chunk=a.chunk, npix=len(lam), n_hr=int(mat.col1 - mat.col0),
               taps_min=int((mat.right - mat.left + 2).min()),
               taps_max=int(mat.W.shape[1]), band_mb=round(mat.W.numel() * 8 / 2**20, 1),
               band_first_ms=round(band[0], 2),
               band_ms=round(float(np.median(band[1:])), 2),
               apply_ms=round(float(np.sum(t_apply)), 2),
               normalize_ms=round(float(np.sum(t_norm)), 2),
               apply_madds=int(nwin) * T,
               apply_tflops=round(2 * nwin * T / (np.sum(t_apply) * 1e-3) / 1e12, 2))
    if a.host:
        hostrows = hr[:1].cpu().numpy().repeat(a.host, axis=0)
        hostrows = torch.as_tensor(hostrows).pin_memory()
        for rep in range(2):
            e0, e1, e2 = ev(), ev(), ev()
            e0.record()
            d = hostrows.to('cuda', non_blocking=True)
            e1.record()
            rows = read_grid.apply_band(mat, d, True)
            make_interpol.normalize_rows(rows, lam, 'linear_continuum', True, 32)
            e2.record()
            torch.cuda.synchronize()
        res.update(host_templates=a.host, host_mb=round(hostrows.numel() * 4 / 2**20, 1),
                   host_copy_ms=round(e0.elapsed_time(e1), 2),
                   host_kernels_ms=round(e1.elapsed_time(e2), 2))
    print(json.dumps(res))


if __name__ == '__main__':
    main()
