"""GPU: the C-ABI drop-ins of the reference's native extension (segmentation/ops/src/vision.cpp:13-16) beyond the fp32 forward of
test_ops_gpu.py: the reference's dtype dispatch (float64 / float16, ms_deform_attn_cuda.cu:64,134) and ms_deform_attn_backward,
against goldens computed by the reference's own ms_deform_attn_core_pytorch (forward) and autograd through it (backward).  The fp16 backward's
packed-pair atomics are held to what they may touch: a misaligned output on the atomics path, and odd element counts (batch = 1), with every output a
sub-view of one tensor the test owns.  (Every kernel instantiation of the backward is held element by element in tests/test_kernel_variants_gpu.py.)"""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def ext():
    import mmsa.msda_ext as e
    return e


def _fwd_args(g, tag, dt):
    return [torch.from_numpy(g[f"{tag}_{k}"]).to(DEV) if k in ("shapes", "lsi") else torch.from_numpy(g[f"{tag}_{k}"]).to(DEV, dt)
            for k in ("value", "shapes", "lsi", "loc", "aw")]


def test_forward_float64_reference_known_answer(ext, golden_dir):
    """The reference's double-precision forward check (ops/test.py:26-50: torch.allclose at default tolerances) through the C ABI."""
    g = np.load(os.path.join(golden_dir, "msda.npz"))
    args = _fwd_args(g, "t", torch.float64)
    out = ext.ms_deform_attn_forward(*args, 2)
    assert out.dtype == torch.float64
    assert torch.allclose(out.cpu(), torch.from_numpy(g["t_out64"]))
    assert (out.cpu() - torch.from_numpy(g["t_out64"])).abs().max() < 1e-15


@pytest.mark.parametrize("tag", ["inj", "ext"])
def test_forward_float16_and_float64_border_cases(ext, golden_dir, tag):
    g = np.load(os.path.join(golden_dir, "msda.npz"))
    ref = torch.from_numpy(g[f"{tag}_out"])
    o64 = ext.ms_deform_attn_forward(*_fwd_args(g, tag, torch.float64), 64)
    assert (o64.cpu().float() - ref).abs().max() <= 2e-6 * ref.abs().max()
    o16 = ext.ms_deform_attn_forward(*_fwd_args(g, tag, torch.float16), 64)
    assert o16.dtype == torch.float16
    # half inputs: the operands are rounded to 11 bits; the reference's own fp32 bar (ops/test.py:53-75) is rtol 1e-2 / atol 1e-3
    assert torch.allclose(o16.cpu().float(), ref, rtol=1e-2, atol=1e-2 * ref.abs().max().item())
    with pytest.raises(RuntimeError):
        ext.ms_deform_attn_forward(*_fwd_args(g, tag, torch.bfloat16), 64)


def _bwd_case(g, tag, dt):
    a = {k: torch.from_numpy(g[f"{tag}_{k}"]) for k in ("value", "shapes", "lsi", "loc", "aw", "gout", "gvalue", "gloc", "gaw")}
    args = [a["value"].to(DEV, dt), a["shapes"].to(DEV), a["lsi"].to(DEV), a["loc"].to(DEV, dt), a["aw"].to(DEV, dt), a["gout"].to(DEV, dt)]
    return args, a


def test_backward_float64_gradcheck_geometry(ext, golden_dir):
    """ms_deform_attn_backward on the geometry of the reference's gradient check (ops/test.py:77-90), float64, against autograd
    through the reference's pytorch core."""
    g = np.load(os.path.join(golden_dir, "msda_bwd.npz"))
    args, a = _bwd_case(g, "t64", torch.float64)
    for got, key in zip(ext.ms_deform_attn_backward(*args, 2), ("gvalue", "gloc", "gaw")):
        assert got.dtype == torch.float64 and tuple(got.shape) == tuple(a[key].shape)
        assert torch.allclose(got.cpu(), a[key], rtol=1e-10, atol=1e-12), key


@pytest.mark.parametrize("tag", ["inj", "ext", "d40"])
def test_backward_float32_border_samples(ext, golden_dir, tag):
    """Border-crossing samples, three levels / one level, and a D = 40 head (not a power of two: the atomics path)."""
    g = np.load(os.path.join(golden_dir, "msda_bwd.npz"))
    args, a = _bwd_case(g, tag, torch.float32)
    outs = ext.ms_deform_attn_backward(*args, 64)
    again = ext.ms_deform_attn_backward(*args, 64)          # outputs are (re)zeroed by the call itself
    for got, got2, key in zip(outs, again, ("gvalue", "gloc", "gaw")):
        ref = a[key]
        assert (got.cpu() - ref).abs().max() <= 2e-5 * ref.abs().max(), key
        assert (got2.cpu() - ref).abs().max() <= 2e-5 * ref.abs().max(), key


def test_backward_float16(ext, golden_dir):
    """Half tensors: the kernel reads the fp16-rounded inputs, computes in fp32 and rounds each gradient once (grad_value: fp16
    atomics).  Expected values = autograd through the oracle's core on the SAME rounded inputs (rounding sampling_loc to 11 bits
    moves samples across pixel / border boundaries, where the location gradient is discontinuous: the fp32 golden of the
    unrounded inputs is not the right comparison for gloc)."""
    from oracle import ref_encoder as R  # checker only
    g = np.load(os.path.join(golden_dir, "msda_bwd.npz"))
    args, a = _bwd_case(g, "inj", torch.float16)
    value, shapes, lsi, loc, aw, gout = [t.cpu() for t in args]
    v32, l32, w32 = value.double().requires_grad_(True), loc.double().requires_grad_(True), aw.double().requires_grad_(True)
    R.msda_core(v32, shapes, l32, w32).backward(gout.double())
    for got, ref, key in zip(ext.ms_deform_attn_backward(*args, 64), (v32.grad, l32.grad, w32.grad), ("gvalue", "gloc", "gaw")):
        assert got.dtype == torch.float16
        ref = ref.float()
        assert (got.cpu().float() - ref).norm() <= 1e-2 * ref.norm(), key


NEG_ZERO = -32768     # the int16 view of fp16 -0.0: a packed-pair atomic that adds +0 to it leaves +0.0 (0)


def _bwd_into_arena(cid, p, starts, refusal_ok=False):
    """mmsa_ms_deform_attn_backward (fp16) with its three outputs placed at the element offsets `starts` of ONE fp16 arena that holds -0.0 everywhere else
    (the outputs themselves start as NaN): every access the kernel can make lies inside an allocation the test owns.  Returns (the arena's bits before,
    the arena after, the output views, reference, bound, slices) -- or, with `refusal_ok`, None after a refusal that left the whole arena as it was."""
    from mmsa import lib, ops
    from tests import variant_ref as V
    i, r, bnd = V.case_data(cid, "msda_bwd", p)
    parts = V.msda_bwd_slices(p)
    levels, lsi, S = V.msda_geometry(p)
    sizes = [s.stop - s.start for s in parts.values()]
    assert all(a + n < b for a, n, b in zip(starts, sizes, list(starts[1:]) + [starts[-1] + sizes[-1] + 8])), "outputs overlap or touch"
    arena = torch.full((starts[-1] + sizes[-1] + 8,), -0.0, dtype=torch.float16, device=DEV)
    assert arena.data_ptr() % 16 == 0
    outs = [arena[a:a + n] for a, n in zip(starts, sizes)]
    for o in outs:
        o.fill_(float("nan"))
    before = arena.view(torch.int16).clone()
    value, loc, aw, gout = (i[k].to(DEV, torch.float16).contiguous() for k in ("value", "loc", "aw", "gout"))
    ss, ls = torch.tensor(levels, dtype=torch.long, device=DEV), torch.tensor(lsi, dtype=torch.long, device=DEV)
    try:
        lib.call("mmsa_ms_deform_attn_backward", value.data_ptr(), ss.data_ptr(), ls.data_ptr(), loc.data_ptr(), aw.data_ptr(), gout.data_ptr(),
                 outs[0].data_ptr(), outs[1].data_ptr(), outs[2].data_ptr(), p["B"], S, p["M"], p["D"], len(levels), p["Lq"], p["P"], 64,
                 ops.MSDA_DTYPES[torch.float16], ops._stream())
    except RuntimeError as e:
        if not refusal_ok:
            raise
        torch.cuda.synchronize()
        assert "aligned" in str(e)
        assert torch.equal(arena.view(torch.int16), before), "a refused call wrote to its outputs"
        return None
    torch.cuda.synchronize()
    return before, arena, outs, r, bnd, parts


def _outside_untouched(before, arena, outs):
    keep = torch.ones(arena.numel(), dtype=torch.bool, device=DEV)
    for o in outs:
        a = o.storage_offset()
        keep[a:a + o.numel()] = False
    got = arena.view(torch.int16)
    assert bool((before[keep] == NEG_ZERO).all())
    return torch.equal(got[keep], before[keep])


@pytest.mark.parametrize("which", ["gloc", "gaw"])
def test_backward_float16_atomics_path_misaligned_output(which):
    """f16 on the atomics path (D = 3): grad_sampling_loc or grad_attn_weight starting at an odd half-word offset.  The packed-pair atomic rounds the
    address down to the aligned pair, so the first element's pair starts one half word before the view.  Either the launcher refuses (and writes
    nothing at all), or everything outside the three views -- the -0.0 half word in front among them -- keeps its bits and the gradients are right.
    (The launcher refuses: the 4-byte alignment check of grad_value covers the other two outputs whenever the atomics path is taken.)"""
    from tests import variant_ref as V
    p = dict(B=2, levels=((5, 7), (3, 2)), P=3, M=3, D=3, Lq=5, dtype="f16")
    nv, nl = 2 * 41 * 3 * 3, 2 * 5 * 3 * 2 * 3 * 2
    starts = [8, 8 + nv + 8 + (which == "gloc"), 8 + nv + 8 + nl + 16 + (which == "gaw")]
    got = _bwd_into_arena("msdab-f16-misaligned", p, starts, refusal_ok=True)
    if got is None:
        return                                         # refused, and nothing was written
    before, arena, outs, r, bnd, parts = got
    assert outs[("gvalue", "gloc", "gaw").index(which)].data_ptr() % 4 == 2
    assert _outside_untouched(before, arena, outs), "memory outside the three outputs changed"
    V.assert_inside(torch.cat(outs), r, bnd, f"misaligned {which}")


@pytest.mark.parametrize("D", [3, 1])
def test_backward_float16_odd_element_counts_leave_the_neighbour_alone(D):
    """batch = 1 with odd S M D (89 * 3 * D) and odd Lq M L P (5 * 3 * 3 * 3), f16, every output 4-byte aligned: the last element of grad_value (and,
    with D = 3 on the atomics path, of grad_attn_weight) sits at an even index, so its packed-pair partner is the half word BEHIND the buffer.  That half
    word holds -0.0 here, like everything else outside the three views, and must hold the same bits after the call: the kernel adds such a last element
    with a 32-bit compare-and-swap that writes the neighbour's bits back unchanged, instead of the packed add of (v, +0) that turned -0.0 into +0.0.
    D = 1 is the shuffle path, whose grad_value goes through the same atomic.  The gradients are held to the float64 bound of tests/variant_ref.py."""
    from tests import variant_ref as V
    p = dict(B=1, levels=((9, 7), (5, 4), (2, 3)), P=3, M=3, D=D, Lq=5, dtype="f16")
    nv, ns = 89 * 3 * D, 5 * 3 * 3 * 3
    assert nv % 2 == 1 and ns % 2 == 1
    starts = [8, 8 + nv + 9, 8 + nv + 9 + 2 * ns + 8]
    before, arena, outs, r, bnd, parts = _bwd_into_arena(f"msdab-f16-odd-d{D}", p, starts)
    assert all(o.data_ptr() % 4 == 0 for o in outs)
    assert float(bnd[parts["gvalue"]][-1]) > 0 and float(bnd[parts["gaw"]][-1]) > 0, "the last elements receive no contribution: the case does not do what it says"
    assert _outside_untouched(before, arena, outs), "memory outside the three outputs changed (the half word behind an odd-sized output?)"
    V.assert_inside(torch.cat(outs), r, bnd, f"odd counts, D = {D}")


def test_autograd_function_matches_reference_gradients(ext, golden_dir):
    """MSDeformAttnFunction (ms_deform_attn_func.py:19-50) end to end: forward value + the three gradients through autograd."""
    g = np.load(os.path.join(golden_dir, "msda_bwd.npz"))
    args, a = _bwd_case(g, "ext", torch.float32)
    value, shapes, lsi, loc, aw, gout = args
    value, loc, aw = value.requires_grad_(True), loc.requires_grad_(True), aw.requires_grad_(True)
    y = ext.MSDeformAttnFunction.apply(value, shapes, lsi, loc, aw, 64)
    y.backward(gout)
    for got, key in ((value.grad, "gvalue"), (loc.grad, "gloc"), (aw.grad, "gaw")):
        assert (got.cpu() - a[key]).abs().max() <= 2e-5 * a[key].abs().max(), key
    assert shapes.grad is None


def test_fused_msda_head_width_40(golden_dir):
    """The hot-path fused gather with D = 40 channels per head (ViT-H: 1280 * 0.5 / 16), 10 lanes per (query, head)."""
    from mmsa import ops
    g = np.load(os.path.join(golden_dir, "msda_bwd.npz"))
    value, shapes, lsi, loc, aw = _fwd_args(g, "d40", torch.float32)
    out = ops.msda_forward(value, shapes, lsi, loc, aw)
    from oracle import ref_encoder as R
    ref = R.msda_core(value.cpu(), shapes.cpu(), loc.cpu(), aw.cpu())
    assert (out.cpu() - ref).abs().max() <= 1e-5 * ref.abs().max()
