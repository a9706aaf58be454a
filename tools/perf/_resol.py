"""Per-spectrum resolution matrices for the measurement tools: 11 diagonals on every
arm, Gaussian rows of sigma 0.45-0.65 A on 0.8-A pixels, normalised -- as resol_ab.py
builds them (what `bench.py --resolution-matrix` puts on its batch)."""
import torch


def attach(batch, S, dev, seed=991):
    """set arm.resol of every arm of `batch` (S spectra) in place"""
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    for a in batch.arms:
        sig = 0.45 + 0.2 * torch.rand((S, 1, 1), device=dev, generator=g,
                                      dtype=torch.float64)
        d = torch.arange(-5, 6, device=dev, dtype=torch.float64)[None, None]
        k = torch.arange(a.npix, device=dev)[None, :, None]
        t = torch.exp(-0.5 * (d / (sig / 0.8))**2).expand(S, a.npix, 11).clone()
        q = k + d.long()
        t = torch.where((q >= 0) & (q < a.npix), t, torch.zeros_like(t))
        t = t / t.sum(dim=2, keepdim=True)
        a.resol = dict(taps=t.contiguous(), nd=11, stride=a.npix * 11,
                       unit=t.sum(dim=2).contiguous())
    return batch
