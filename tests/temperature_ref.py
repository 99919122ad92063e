"""Float64 references, bounds and inputs the temperature-scaling tests share (csrc/softmax_px.h softmax_px_exp_t, csrc/temperature.hip) -- TEST
INFRASTRUCTURE ONLY.  The references are formed from float64(x) * float64(it) with `it` the float32 inverse temperature the kernels multiply by
(mmsa.evaluate.inv_temperature), on the SAME float32 canvas logits; the bounds are the ones DESIGN.md section 2 derives, never measured ones."""
import numpy as np
import torch

NLL_ONE = 2 ** 20


def scaled64(x, it):
    """float64(x) * float64(it), [B, C, H, W] on the host."""
    return x.double().cpu() * float(np.float64(np.float32(it)))


def spread(x, it):
    """D_T = max_c |x_c - m| * it per pixel, float64 [B, H, W]."""
    z = scaled64(x, it)
    return (z - z.max(1, keepdim=True).values).abs().max(1).values


def confidence_check(conf, x, it):
    """conf float32 [B, H, W] against max_c softmax(float64(x) * float64(it)) -> (worst relative error / bound, largest D_T).  The bound per pixel is
    (4 D_T + C + 4) 2^-23: the confidence bound of tests/confidence_ref.py with TWO roundings entering the exponent (x - m, then the product with it)."""
    z = scaled64(x, it)
    C = z.shape[1]
    want = torch.softmax(z, dim=1).max(1).values
    D = spread(x, it)
    bound = (4 * D + C + 4) * 2.0 ** -23
    rel = (conf.double().cpu() - want).abs() / want
    return (rel / bound).max().item(), D.max().item()


def nll64(x, it, cls):
    """-log_softmax(float64(x) * float64(it))[cls] per pixel, float64 [B, H, W]; `cls` int64 [B, H, W] class indices (any value where a pixel takes no part:
    it is clamped for the gather and the caller masks)."""
    z = scaled64(x, it)
    ls = torch.log_softmax(z, dim=1)
    return -ls.gather(1, cls.clamp(0, z.shape[1] - 1).unsqueeze(1).cpu()).squeeze(1)


def nll_sum_bound(x, it, cls, part):
    """(sum of nll64 over the participating pixels, the bound on |sum n / 2^20 - that sum|): per pixel (4 D_T + C + 4 + nll64) 2^-23 + 2^-20 -- the bound of
    the sum of exponentials, one ulp of logf, the rounded product and subtraction, and the floor to 20 fractional bits."""
    n64 = nll64(x, it, cls)
    C = x.shape[1]
    per = (4 * spread(x, it) + C + 4 + n64) * 2.0 ** -23 + 2.0 ** -20
    part = part.cpu()
    return n64[part].sum().item(), per[part].sum().item(), n64[part].max().item() if bool(part.any()) else 0.0


def labels_for(B, Hl, Wl, C, seed, ignored=0.1, out_of_range=0.1):
    """Raw uint8 label maps [B, Hl, Wl]: classes 0 .. C - 1, a share of 255 (ignored) and -- where the byte has room -- a share of kept values in
    [C, 254] (kept but out of range: they take no part either)."""
    g = torch.Generator().manual_seed(seed)
    lab = torch.randint(0, C, (B, Hl, Wl), generator=g)
    r = torch.rand(B, Hl, Wl, generator=g)
    lab[r < ignored] = 255
    if C < 254:
        oor = torch.randint(C, 255, (B, Hl, Wl), generator=g)
        lab = torch.where((r >= ignored) & (r < ignored + out_of_range), oor, lab)
    return lab.to(torch.uint8)


def planted_temperature_case():
    """A canvas whose labels were DRAWN from softmax(z) and whose logits are x = 2.5 z: the fit must find T = 2.5.  -> (x float32 [2, 5, 37, 83], labels
    uint8 [2, 37, 83], the grid).  Generator use in this order: randn, then multinomial."""
    g = torch.Generator().manual_seed(0)
    z = torch.randn(2, 5, 37, 83, generator=g) * 2
    p = torch.softmax(z.double(), dim=1).permute(0, 2, 3, 1).reshape(-1, 5)
    lab = torch.multinomial(p, 1, generator=g).reshape(2, 37, 83).to(torch.uint8)
    x = (2.5 * z).float()
    return x, lab, (0.5, 1.0, 1.75, 2.5, 3.5, 5.0)


def planted_float64(x, lab, grid, bins=15):
    """Mean NLL and ECE over the grid in float64 on the host (equal-width bins, the last one closed) -> (nll [J], ece [J])."""
    nll, ece = [], []
    cls = lab.long()
    for T in grid:
        z = x.double() / T
        ls = torch.log_softmax(z, dim=1)
        nll.append(float(-ls.gather(1, cls.unsqueeze(1)).mean()))
        conf, pred = ls.exp().max(1)
        ok = (pred == cls).double()
        k = torch.clamp((conf * bins).long(), max=bins - 1)
        e = 0.0
        for b in range(bins):
            sel = k == b
            if bool(sel.any()):
                e += float(sel.double().mean()) * abs(float(ok[sel].mean()) - float(conf[sel].mean()))
        ece.append(e)
    return np.array(nll), np.array(ece)
