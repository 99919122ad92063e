"""One-time weight preprocessing of the backbone: a state dict becomes the packed tree the forward reads (operand planes, folded norms, re-laid-out
conv weights).  `PackPlan` decides -- as plain Python, testable without a device -- which operand format every GEMM site gets and which LayerNorm folds
apply; the `pack_*` functions of (sd, plan, dev) build one part of the tree each; `pack(model, dev)` assembles them."""
import collections

import torch

from . import ops


class PackPlan(collections.namedtuple("PackPlan", "cfg channels depths sites h8c cnx_f16_on fold_ln_on share_c_norm fold_adapter_ln_on fold_cnx_ln fp8_weights wide inter_pairs")):
    """Everything the packed tree depends on besides the weights: the architecture, the model's numerics attributes (`sites` = `h8_sites` as configured, the `*_on` fields = the attributes before
    the shape rules below; `h8c`: h8 sites with deep contractions travel as h8c planes (default), `model.h8c = False` keeps them on h8 line planes for the A/B) and its two sticky states
    (`wide`, `inter_pairs`)."""
    __slots__ = ()

    @classmethod
    def of(cls, m):
        g = lambda k, d: bool(getattr(m, k, d))   # noqa: E731
        return cls(m.cfg, tuple(m.channels), tuple(m.depths), tuple(getattr(m, "h8_sites", m.H8_DEFAULT)), g("h8c", True), g("cnx_f16", True), g("fold_ln", True),
                   g("share_c_norm", True), g("fold_adapter_ln", False), g("fold_convnext_ln", False), g("fp8_weights", False), g("_wide_range", False),
                   frozenset(getattr(m, "_inter_pairs", ()) or ()))

    D = property(lambda s: s.cfg["embed_dim"])
    heads = property(lambda s: s.cfg["num_heads"])
    hd_true = property(lambda s: s.D // s.heads)
    hd_pad = property(lambda s: ops.pad32(s.hd_true))     # head width the kernels see (zero-padded to the 32-wide MFMA k-block: pack_vit)
    Da = property(lambda s: s.heads * s.hd_pad)           # attention width (= D unless padded)
    hidden = property(lambda s: int(s.D * s.cfg["mlp_ratio"]))
    hid_c = property(lambda s: int(s.D * s.cfg["cffn_ratio"]) if s.cfg["with_cffn"] else 128)

    @property
    def h8_sites(self):   # wide-range state: no GEMM site on fp16-based planes ("attnv", the attention kernels' own operands, stays)
        return tuple(s_ for s_ in self.sites if s_ not in ("vit", "inter", "up", "cnx", "cnx2")) if self.wide else self.sites

    @property
    def pair_fmt(self):
        """The hi/lo PAIR format of the ViT-block GEMMs (h8 off, or a block moved off single fp16 operands by the logit guard): fp16 pairs (f3: 22
        significant bits, +-65504), or bf16 pairs (16 bits, fp32's range) in the wide-range state."""
        return ops.FMT_B3 if self.wide else ops.FMT_F3

    def block_fmt(self):
        """Operand format of the ViT-block GEMMs: h8 needs every contraction length (D, attention width, MLP hidden) % 64 == 0 ... as h8c planes (3 bytes per element, csrc/gemm_h8c.hip: a shorter
        operand stream and balanced matrix phases) where every contraction of the block is at least 512 deep (few k-tile pairs per output tile leave that kernel's straight-line loop
        nothing to run), h8 line planes otherwise; else the pair format, fp16 hi/lo pairs like the attention kernels' own.  fp8_weights needs the blocks on h8c planes: ValueError (at pack
        time) where they would not run there."""
        D, Da, hidden = self.D, self.Da, self.hidden
        fmt = self.pair_fmt
        if "vit" in self.h8_sites and D % 64 == 0 and Da % 64 == 0 and hidden % 64 == 0:
            fmt = ops.FMT_H8C if (min(D, Da, hidden) >= 512 and self.h8c) else ops.FMT_H8
        if self.fp8_weights:
            # (judged on the configured sites: the wide-range state keeps the fp8 values on bf16 pairs, with the same effective weights)
            why = ("'vit' is not among h8_sites" if "vit" not in self.sites else "h8c is off" if not self.h8c
                   else f"a contraction is shorter than 512 (embed {D}, attention width {Da}, MLP hidden {hidden})" if min(D, Da, hidden) < 512
                   else f"a contraction is not a multiple of 128 (embed {D}, attention width {Da}, MLP hidden {hidden})" if (D % 128 or Da % 128 or hidden % 128)
                   else None)
            if why:
                raise ValueError(f"mmsa: fp8_weights needs the ViT-block GEMMs on h8c planes, but {why}")
            if fmt == ops.FMT_H8C:
                fmt = ops.FMT_W8
        return fmt

    def inter_fmt(self, k, index=None, site="inter", h8c_ok=True):
        """Operand format of one GEMM of contraction length `k` of a site group ("inter": of interaction `index`; "up"): h8c / h8 when the site is selected
        and the contraction length allows it.  `h8c_ok=False`: the producer of the A operand cannot write h8c (ConvFFN fc2, pack_interactions)."""
        kk = ops.pad32(k)
        if site == "inter" and index in self.inter_pairs and site in self.h8_sites:
            return self.pair_fmt             # this interaction follows its blocks onto hi/lo pairs (inter_follow_blocks)
        if site not in self.h8_sites or kk % 64:
            return ops.FMT_B3
        return ops.FMT_H8C if (h8c_ok and kk >= 512 and self.h8c) else ops.FMT_H8

    @property
    def cnx_f16(self):
        """TwinConvNeXt GEMMs on fp16 hi/lo pairs (default) instead of bf16 hi/lo; `model.cnx_f16 = False` for the A/B.  Not with the opt-in ConvNeXt
        LayerNorm fold (its depthwise kernel writes bf16 hi/lo planes), not in the wide-range state."""
        return self.cnx_f16_on and not self.fold_cnx_ln and not self.wide

    def cnx_fmt(self, c, pw=0):
        """Operand format of the TwinConvNeXt GEMMs of a stage of width `c`: pw = 1 / 2 its pointwise convs, 0 the stem / downsample convs."""
        # "cnx" in h8_sites (NOT a default: the 36-block chain is the error-sensitive part of the path, LAB_NOTES.md section 2): h8 operands for the pointwise convs whose two contraction lengths
        # (C and 4C) are multiples of 64 and that do not run on the fused stage-0 kernel ("cnx2": stage 2 alone -- the selective variant of tools/cnx_h8_study.py, measured and left off:
        # LAB_NOTES.md section 4.2)
        sites = self.h8_sites
        if pw and ("cnx" in sites or ("cnx2" in sites and c == self.channels[2])) and c % 64 == 0 and not ops.convnext_mlp_fused_supported(c):
            return ops.FMT_H8
        # "cnx2p2" (round 6; NOT a default): pointwise_conv2 of stage 2 alone (K = 4C = 1536: 12 k-tile pairs, the h8c kernel's regime) on h8c planes -- two matrix units per
        # product instead of three; pointwise_conv1 stays on f3 and writes its GELU output as h8c planes. tools/cnx_precision_trade.py + profiles/r06_cnx_precision_trade.txt: f3 / f4 error x 2 / x
        # 3.5 at ViT-B on the oracle for the step time measured there
        if "cnx2p2" in sites and pw == 2 and c == self.channels[2] and (4 * c) % 64 == 0 and 4 * c >= 512 and self.h8c:
            return ops.FMT_H8C
        # default (round 4): fp16 hi/lo pairs ("f3": 22 significant bits, the same three MFMAs per product as bf16 hi/lo) for the whole
        # chain (stem, downsample and pointwise convs) -- its operand rounding is what GFFM amplifies (LAB_NOTES.md section 2, tools/f3_study.py)
        return ops.FMT_F3 if self.cnx_f16 else ops.FMT_B3

    @property
    def fold_ln(self):
        """LayerNorm fold (IE:396-421; LAB_NOTES.md 4.2): norm1 / norm2 of the ViT blocks live in their consumer GEMMs.  The producer of the residual stream (proj, lin2, the injector's output
        projection) also writes the stream as planes and per-row strip sums; qkv / lin1 run on W o w and compute rstd * (x W'^T - mean * colsum(W')) + (W b + bias) in their epilogue.
        tools/lnfold_study.py: same error as LayerNorm + GEMM on the seeded weights, + 1.5e-5 at |mean| = 4.5 std.  Needs whole 128-column tiles and 64-column strips."""
        return self.fold_ln_on and self.D % 64 == 0 and (3 * self.Da) % 128 == 0 and self.hidden % 128 == 0

    def fold_cnx(self, c):
        """ConvNeXt LayerNorm fold (round 3) for a stage of width `c`: OPT-IN (`model.fold_convnext_ln = True`).  Built, tested, and measured at ViT-L 1024^2: step -0.17 ms, golden probes 2.9e-4
        -> 4.6e-4 (the chain's error is amplified ~15 x by GFFM, LAB_NOTES.md sections 2 and 4.2): not worth the margin.  Applies to the stages that run pointwise_conv1 as a GEMM (not the
        fused stage-0 pair), 64-channel chunks."""
        return self.fold_cnx_ln and c % 64 == 0 and (4 * c) % 128 == 0 and not ops.convnext_mlp_fused_supported(c)

    @property
    def fold_adapter_ln(self):
        """Round 5: the adapter tokens' LayerNorms inside their consumer GEMMs (`fold_adapter_ln`; the ViT blocks' fold of round 3 applied to AM:490-511,525-542). Every LayerNorm over c -- the
        shared injector feat_norm / extractor query_norm, the extra extractors' query_norm, every ffn_norm -- follows a GEMM that has just written c (ConvFFN fc2, the extractor's output
        projection).  That producer also writes c's RAW operand planes and per-row strip sums; mmsa_rowstats_finalize turns them into (mean, rstd); the consumers (value / offsets
        projections, fc1) run on W o w with the row-normalising epilogue. Twelve passes over the largest token matrix of the path (21504 x 1024 per image: 88 MB read + 66 MB planes written
        each) go away.  Needs the affine parts folded into the weights (share_c_norm) and whole 128-column tiles at every consumer; tools/lnfold_adapter_study.py: no measurable error.
        OPT-IN (`model.fold_adapter_ln = True`): built, pinned against the oracle (tests/test_backbone_gpu.py::test_adapter_layernorm_fold_against_the_oracle), and measured step-NEUTRAL at
        ViT-L 1024^2 (profiles/r05_adapter_ln_fold.txt: 31.12 / 31.39 ms without, 31.41 / 31.34 ms with; golden probes 0.94e-4 -> 1.15e-4): the eleven passes it deletes cost what the
        producers' extra plane + strip-sum stores and the consumers' row loads cost -- by bytes the fold saves only the read of c (176 MB per pass at batch 2), 0.3 ms at best.  A pack-time
        setting that drives the run-time path."""
        return (self.share_c_norm and self.fold_adapter_ln_on and "inter" in self.h8_sites and self.D % 64 == 0
                and int(self.D * self.cfg["deform_ratio"]) % 128 == 0 and self.hid_c % 128 == 0
                and not self.inter_pairs)   # (the fold hands c's planes from one interaction's producer to the next one's consumers: one format for all)

    def settings(self):
        """The pack-time settings the planes depend on, as packed files (checkpoint.PACK_FORMAT 12) carry them under "settings": a pack made with other
        settings is stale (backbone._prepare), a file refused (checkpoint.load_packed)."""
        s = {"h8_sites": list(self.h8_sites), "h8c": self.h8c, "share_c_norm": self.share_c_norm, "fold_ln": self.fold_ln, "fold_cnx_ln": self.fold_cnx_ln,
             "cnx_f16": self.cnx_f16, "fold_adapter_ln": self.fold_adapter_ln, "wide": self.wide, "inter_pairs": sorted(self.inter_pairs)}
        if self.fp8_weights:   # (fp8 packs only: the ViT-block weights are W8 codes + exponents; a file without the key was packed without the switch)
            s["fp8_weights"] = True
        return s


def packed_settings(pk):
    """PackPlan.settings() of the plan a packed tree was made with, read back from the tree (which stores them under the same names)."""
    s = {"h8_sites": list(pk["h8_sites"]), "inter_pairs": list(pk["inter_pairs"])}
    s.update((k, bool(pk[k])) for k in ("h8c", "share_c_norm", "fold_ln", "fold_cnx_ln", "cnx_f16", "fold_adapter_ln", "wide"))
    return dict(s, fp8_weights=True) if pk.get("fp8_weights") else s


def fold_gfe_qkv(q1, q2, q1_bias=None, groups=32):
    """The GFE's qkv2(qkv1(x)) (AM:87-92: grouped 1x1 conv c -> 3c, then grouped 3x3 conv 3c -> 3c, the same groups, no bias, nothing in between) is itself a grouped 3x3 conv c -> 3c: group g of
    qkv2 reads exactly the channels group g of qkv1 wrote, and zero padding commutes with a bias-free 1x1 conv, so the border pixels are exact too.  From the module weights q1 [3c, c/G, 1, 1]
    and q2 [3c, 3c/G, 3, 3] returns W_eff[g][tap][ci][co] = sum_m q1[g][ci][m] q2[g][tap][m][co], summed in float64 and rounded once to fp32 -- the layout of the packed `q2` (ops.gfe_qkv).
    With a qkv1 bias the padded border of qkv2 would see zeros where the composition sees the bias: no fold, returns None."""
    if q1_bias is not None:
        return None
    G = groups
    co, ci = q1.shape[0] // G, q1.shape[1]
    a = q1.detach().double().reshape(G, 1, co, ci).transpose(2, 3)            # [G][1][ci][m]
    b = q2.detach().double().reshape(G, co, co, 9).permute(0, 3, 2, 1)        # [G][tap][m][co]
    return torch.matmul(a, b).float().contiguous()                             # [G][tap][ci][co]


def _linear_resize_rows(tab, L):
    """F.interpolate(mode='linear', align_corners=False) along dim 0 of a [Lin, C] table (IE:568-575)."""
    Lin = tab.shape[0]
    scale = Lin / L
    pos = (torch.arange(L, dtype=torch.float32, device=tab.device) + 0.5) * scale - 0.5
    pos = pos.clamp(min=0)
    i0 = pos.floor().long().clamp(max=Lin - 1)
    i1 = (i0 + 1).clamp(max=Lin - 1)
    lam = (pos - i0.float()).unsqueeze(1)
    return tab[i0] * (1 - lam) + tab[i1] * lam


def fp8_effective(w, lnw=None):
    """fp8 weights: (what the kernel multiplies by -- 2^e e4m3(W o lnw), exact in fp32 --, the same in the reference's parameterisation: that / lnw,
    and W itself in a column whose LayerNorm weight is 0, which then contributes through the LayerNorm bias alone -- consistently in the folded bias)."""
    if lnw is None:
        q = ops.fp8_dequantize(*ops.fp8_quantize(w))
        return q, q
    q = ops.fp8_dequantize(*ops.fp8_quantize(w * lnw[None, :]))
    nz = lnw[None, :] != 0
    return q, torch.where(nz, q / torch.where(nz, lnw[None, :], torch.ones_like(lnw[None, :])), w)


def float_state_dict(model, dev):
    """The float parameters on `dev`, plus ZERO stand-ins for the tensors a ViT built with qkv_bias=False / use_rel_pos=False does not
    have (IE:317,320-327): a zero qkv bias and zero rel-pos tables make the kernels compute exactly what the reference computes
    without them (the pad tokens' k / v = bias = 0; rel_pos . q = 0 added to the logits)."""
    sd = {k: v.detach().to(dev, torch.float32) for k, v in model.state_dict().items() if v.dtype.is_floating_point}
    cfg = model.cfg
    D, hd = cfg["embed_dim"], cfg["embed_dim"] // cfg["num_heads"]
    grid = cfg["pretrained_size"] // cfg["patch_size"]
    for i in range(cfg["depth"]):
        b = f"blocks.{i}.attn."
        if not cfg["qkv_bias"]:
            sd[b + "qkv.bias"] = torch.zeros(3 * D, device=dev)
        if not cfg["use_rel_pos"]:
            L = 2 * (grid if i in cfg["global_attn_indexes"] else cfg["window_size"]) - 1
            sd[b + "rel_pos_h"] = torch.zeros(L, hd, device=dev)
            sd[b + "rel_pos_w"] = torch.zeros(L, hd, device=dev)
    return sd


def _planes(w2d, kpad=None, fmt=ops.FMT_B3):
    if fmt == ops.FMT_W8:
        return ops.w8_planes(w2d.contiguous())
    return ops.split_planes(w2d.contiguous(), kpad, fmt=fmt, weight=fmt == ops.FMT_H8)


def pad_head_rows(w, groups, plan):
    """[groups*heads*hd_true, ...] -> [groups*heads*hd_pad, ...]: zero rows for the pad channels of every head"""
    heads, hd_true, hd = plan.heads, plan.hd_true, plan.hd_pad
    if hd == hd_true:
        return w.contiguous()
    v = w.reshape(groups, heads, hd_true, *w.shape[1:])
    out = v.new_zeros(groups, heads, hd, *w.shape[1:])
    out[:, :, :hd_true] = v
    return out.reshape(groups * heads * hd, *w.shape[1:]).contiguous()


def _pad_rows128(w, b):   # zero rows (and bias entries) up to whole 128-column GEMM tiles
    npad = -w.shape[0] % 128
    return (torch.cat([w, w.new_zeros(npad, w.shape[1])], 0), torch.cat([b, b.new_zeros(npad)], 0)) if npad else (w, b)


def fold_ln_planes(w, bias, lnw, lnb, fmt, fp8=False, f64=True, pad128=False, colsums=True):
    """A projection W x + bias behind LayerNorm(.; lnw, lnb), folded: (planes of W o lnw, the column sums of those planes as the kernel will read them -- what every x_k is actually multiplied
    with, summed in float64 --, W lnb + bias).  `fp8`: of the effective fp8 weights.  `f64`: the bias product in float64 (the ViT and ConvNeXt folds; the adapter fold's is the fp32 bias + W
    lnb it has had since round 2, kept to the bit).  `pad128`: _pad_rows128."""
    wk, w = fp8_effective(w, lnw) if fp8 else (w * lnw[None, :], w)
    bf = (w.double() @ lnb.double()).float().add_(bias) if f64 else bias + w @ lnb
    if pad128:
        wk, bf = _pad_rows128(wk.contiguous(), bf.contiguous())
    pl = _planes(wk, fmt=fmt)
    cs = ops.planes_to_float(pl, cols=pl.k)[: pl.n].double().sum(1).float().contiguous() if colsums else None
    return pl, cs, bf.contiguous()


# ---------------------------------------------------------------------------------------------- ViT
@torch.no_grad()
def block_gemm_planes(sd, plan, i, fmt, fold, dev):
    """The four GEMM weights of ViT block i as operand planes of format `fmt` (+ the LayerNorm-folded forms of qkv / lin1 when
    `fold`): head widths that are not a multiple of 32 zero-padded per head (ViT-H), see pack_vit."""
    fp8 = plan.fp8_weights   # (fmt = FMT_W8, or a pair format in the guard's / wide-range state's repacks: the same effective weights)

    plain = lambda w: _planes(fp8_effective(w)[0] if fp8 else w, fmt=fmt)   # noqa: E731
    b = f"blocks.{i}."
    g = lambda k: sd[b + k].detach().to(dev, torch.float32)   # noqa: E731
    qkv_w, qkv_bias = pad_head_rows(g("attn.qkv.weight"), 3, plan), pad_head_rows(g("attn.qkv.bias"), 3, plan)
    proj_w = pad_head_rows(g("attn.proj.weight").t(), 1, plan).t().contiguous()    # zero COLUMNS for the pad channels
    skip = fp8 and fold   # (fp8: the unfolded qkv / lin1 would be quantized only to be replaced)
    out = dict(qkv=None if skip else plain(qkv_w), proj=plain(proj_w), lin1=None if skip else plain(g("mlp.lin1.weight")), lin2=plain(g("mlp.lin2.weight")))
    if fold:   # the consumers' weights carry their LayerNorm (the unfolded planes are not kept: the fold is all or nothing per model)
        out["qkv"], out["qkv_cs"], out["qkv_bf"] = fold_ln_planes(qkv_w, qkv_bias, g("norm1.weight"), g("norm1.bias"), fmt, fp8)
        out["lin1"], out["lin1_cs"], out["lin1_bf"] = fold_ln_planes(g("mlp.lin1.weight"), g("mlp.lin1.bias"), g("norm2.weight"), g("norm2.bias"), fmt, fp8)
    return out


def block_static(sd, plan, i):
    """Everything of ViT block i but its four GEMM weights: norms, biases, the qkv bias rows as planes, the rel-pos tables."""
    cfg, Da, hd, hd_true, attnv = plan.cfg, plan.Da, plan.hd_pad, plan.hd_true, "attnv" in plan.h8_sites
    b = f"blocks.{i}."

    pad_cols = lambda t: t if hd == hd_true else torch.cat([t, t.new_zeros(t.shape[0], hd - hd_true)], 1)   # noqa: E731  [L, hd_true] -> [L, hd]
    qkv_bias = pad_head_rows(sd[b + "attn.qkv.bias"], 3, plan)
    row = qkv_bias.reshape(1, -1).contiguous()
    return dict(
        n1w=sd[b + "norm1.weight"], n1b=sd[b + "norm1.bias"], n2w=sd[b + "norm2.weight"], n2b=sd[b + "norm2.bias"],
        qkv_b=qkv_bias,
        # k = v of pad tokens; with the fp16 P V of the attention kernels (the "attnv" site, a default; `h8_sites` without it: fp16 hi/lo pairs) the v third
        # of the qkv planes -- these bias rows and the qkv GEMM's output -- is h8-encoded (ops.Planes.split)
        qkv_bp=(ops.split_planes_qkv(row, Da) if (attnv and Da % 32 == 0) else ops.split_planes(row, kpad=3 * Da, fmt=ops.FMT_F3)),
        # ... and for the kernels with the rel-pos terms fused (head_dim 64) the whole row, the qkv GEMM's whole output and the
        # rel-pos tables are h8 planes: every contraction of those kernels runs on the fp16 hi parts (v_fmt = 2)
        qkv_bp16=(ops.split_planes(row, kpad=3 * Da, fmt=ops.FMT_H8) if attnv else None),
        # ... and plain bf16 hi/lo planes for a block whose logit range rules fp16 operands out (attention_precision, _attn_mode)
        qkv_bp_b3=ops.split_planes(row, kpad=3 * Da, fmt=ops.FMT_F3),
        proj_b=sd[b + "attn.proj.bias"], lin1_b=sd[b + "mlp.lin1.bias"], lin2_b=sd[b + "mlp.lin2.bias"],
        rph=pad_cols(sd[b + "attn.rel_pos_h"]), rpw=pad_cols(sd[b + "attn.rel_pos_w"]),
        ws=0 if i in cfg["global_attn_indexes"] else cfg["window_size"], index=i)


def pack_vit(sd, plan, dev):
    """Patch embedding and the ViT blocks.  Head widths that are not a multiple of the 32-wide MFMA k-block (ViT-H: 1280 / 16 = 80) run ZERO-PADDED per head (80 -> 96): the qkv projection gets
    zero rows (and zero bias) for the pad channels, the output projection zero columns, the rel-pos tables zero columns.  q.k, the rel-pos terms and the proj output are unchanged -- every
    added term is an exact zero -- and the softmax scale stays head_dim^-0.5 of the true width."""
    vfmt, fold = plan.block_fmt(), plan.fold_ln
    blocks = []
    for i in range(plan.cfg["depth"]):
        blk = block_static(sd, plan, i)
        blk.update(block_gemm_planes(sd, plan, i, vfmt, fold, dev))
        wsz = blk["ws"]
        if wsz and wsz <= 14 and plan.hd_pad == 64:   # windowed blocks with head_dim 64: rel-pos tables packed for the fused window kernel
            L = 2 * wsz - 1
            th = blk["rph"] if blk["rph"].shape[0] == L else _linear_resize_rows(blk["rph"], L)
            tw = blk["rpw"] if blk["rpw"].shape[0] == L else _linear_resize_rows(blk["rpw"], L)
            blk["relp"] = ops.window_relpos_planes(th, tw, wsz, fmt=ops.FMT_F3)
            blk["relp16"] = ops.window_relpos_planes(th, tw, wsz, fmt=ops.FMT_H8) if blk["qkv_bp16"] is not None else None
        blocks.append(blk)
    return dict(pe_w=_planes(sd["patch_embed.proj.weight"].reshape(plan.D, -1)),  # K order (c,kh,kw)
                pe_b=sd["patch_embed.proj.bias"].contiguous(), blocks=blocks, fp8_weights=plan.fp8_weights, vit_fmt=vfmt, fold_ln=fold)


def repack_block_on_pairs(pk, bp, sd_dev, plan, dev):
    """Move the four GEMMs of block `bp` to the pair format (nothing to do where they are on it already): a block on pair attention runs its
    projections on pairs too (backbone.check_attention_guard).  `sd_dev`: a function returning float_state_dict (called only when a block moves)."""
    if bp["qkv"].fmt != plan.pair_fmt:
        bp.update(block_gemm_planes(sd_dev(), plan, bp["index"], plan.pair_fmt, pk["fold_ln"], dev))


def carry_block_modes(pk, modes, sd_dev, plan, dev):
    """The blocks' settled attention precision into a fresh pack.  `modes`: per block a dict with the `amode` / `max_logit` it has settled (a block
    that had none gets none), in the order the tree is to hold them; a block on pair attention ("b3") moves its four GEMMs to pairs as well."""
    for bp, m in zip(pk["blocks"], modes):
        bp.update(m)
        if m.get("amode") == "b3":
            repack_block_on_pairs(pk, bp, sd_dev, plan, dev)


# ---------------------------------------------------------------------------------------------- TwinConvNeXt
def _stack2(fx, fy):
    if isinstance(fx, dict):
        return {k: _stack2(fx[k], fy[k]) for k in fx}
    if isinstance(fx, (list, tuple)):
        return [_stack2(u, v) for u, v in zip(fx, fy)]
    if isinstance(fx, ops.Planes):
        buf = torch.cat([fx.p, fy.p], 0).contiguous()
        pl = ops.Planes(buf[:fx.p.shape[0]], fx.n, fx.k, fx.kpad, fx.fmt, fx.weight)    # (h8c planes hold row PAIRS: n / 2 tensor rows)
        pl.full = buf           # keeps the second batch alive; batch stride = Planes.batch_stride(n)
        return pl
    return torch.stack([fx, fy], 0).contiguous()


def pack_twin(sd, plan, dev):
    """Both ConvNeXt streams stacked along a leading batch dimension: the two chains run as ONE chain of batched kernels (per-batch weights), see
    backbone._twin_batched.  Only the stacked form is used by the forward (and written by checkpoint.save_packed)."""
    t = "spm.twin_conv."
    ch, f0 = plan.channels, plan.cnx_fmt(plan.channels[0])
    twin = {}
    for s in ("x", "y"):
        d = t + f"downsample_layers_{s}."
        st = dict(stem=_planes(sd[d + "0.0.weight"].reshape(ch[0], -1), fmt=f0), stem_b=sd[d + "0.0.bias"],
                  stem_nw=sd[d + "0.1.weight"], stem_nb=sd[d + "0.1.bias"], ds=[], stages=[], out_norm=[])
        for i in range(1, 4):
            w = sd[d + f"{i}.1.weight"]  # [Cout, Cin, 2, 2] -> K order (kh, kw, cin)
            st["ds"].append(dict(nw=sd[d + f"{i}.0.weight"], nb=sd[d + f"{i}.0.bias"],
                                 w=_planes(w.permute(0, 2, 3, 1).reshape(w.shape[0], -1), fmt=f0), b=sd[d + f"{i}.1.bias"]))
        for i in range(4):
            blks = []
            f1, f2 = plan.cnx_fmt(ch[i], 1), plan.cnx_fmt(ch[i], 2)
            for j in range(plan.depths[i]):
                b = t + f"stages_{s}.{i}.{j}."
                dw = sd[b + "depthwise_conv.weight"]  # [C,1,7,7] -> tap-major [49, C]
                w1 = sd[b + "pointwise_conv1.weight"]
                blk = dict(dw=dw.reshape(dw.shape[0], 49).t().contiguous(), dw_b=sd[b + "depthwise_conv.bias"],
                           nw=sd[b + "norm.weight"], nb=sd[b + "norm.bias"],
                           pw1=_planes(w1, fmt=f1), pw1_b=sd[b + "pointwise_conv1.bias"],
                           pw2=_planes(sd[b + "pointwise_conv2.weight"], fmt=f2), pw2_b=sd[b + "pointwise_conv2.bias"],
                           gamma=sd[b + "gamma"])
                if plan.fold_cnx(ch[i]):
                    # the block's LayerNorm (TC:103-106) folded into pointwise_conv1: W o w as planes, their column sums as the kernel
                    # reads them, W b + bias (the depthwise conv writes the RAW planes + strip sums, _spm)
                    blk["pw1f"], blk["pw1_cs"], blk["pw1_bf"] = fold_ln_planes(w1, sd[b + "pointwise_conv1.bias"], sd[b + "norm.weight"], sd[b + "norm.bias"], f1)
                blks.append(blk)
            st["stages"].append(blks)
            st["out_norm"].append((sd[t + f"norm_{s}{i}.weight"], sd[t + f"norm_{s}{i}.bias"]))
        twin[s] = st
    return _stack2(twin["x"], twin["y"])


# ---------------------------------------------------------------------------------------------- fusion neck
def pack_neck(sd, plan, dev):
    D = plan.D
    f = "spm.smart_fusion."

    scalar = lambda k: float(sd[k].item())   # noqa: E731
    neck = []
    for i in range(4):
        c = plan.channels[i]
        C = 2 * c
        lv = dict(gfe=[], loc=[])
        for m in ("rgb", "sne"):
            b = f + f"global_feature_encoder_{m}.{i}."
            q1 = sd[b + "attn.qkv1.weight"]  # [3c, c/32, 1, 1], groups 32 -> [G][tap][ci][co]
            q2 = sd[b + "attn.qkv2.weight"]  # [3c, 3c/32, 3, 3]
            G = 32
            co1, ci1, co2, ci2 = 3 * c // G, c // G, 3 * c // G, 3 * c // G
            lv["gfe"].append(dict(
                nw=sd[b + "norm1.body.weight"], nb=sd[b + "norm1.body.bias"],
                q1=q1.reshape(G, co1, ci1, 1).permute(0, 3, 2, 1).contiguous(),
                q2=q2.reshape(G, co2, ci2, 9).permute(0, 3, 2, 1).contiguous(),
                temp=sd[b + "attn.scale"].reshape(8).contiguous(), scale2=scalar(b + "attn.scale2"),
                proj=sd[b + "attn.proj.weight"].reshape(c, c).contiguous()))
            q12 = fold_gfe_qkv(q1, q2, sd.get(b + "attn.qkv1.bias"), G)   # (q1 / q2 stay: shapes the fused kernel does not cover, fuse_gfe_qkv = False)
            if q12 is not None:
                lv["gfe"][-1]["q12"] = q12
            b = f + f"local_feature_encoder_{m}.{i}."
            dw = sd[b + "bottleneckBlock.2.weight"]
            lv["loc"].append(dict(
                w1=_planes(sd[b + "bottleneckBlock.0.weight"].reshape(2 * c, c)),
                dw=dw.reshape(2 * c, 9).t().contiguous(),
                w3=_planes(sd[b + "bottleneckBlock.4.weight"].reshape(c, 2 * c)), scale=scalar(b + "scale")))
        b = f + f"fuse_blocks.{i}."
        lv["gx"], lv["gy"] = scalar(b + "gammax.scale"), scalar(b + "gammay.scale")
        lv["lnw"], lv["lnb"] = sd[b + "norm.weight"].contiguous(), sd[b + "norm.bias"].contiguous()
        lv["lnw_mean"], lv["lnb_mean"] = float(lv["lnw"].double().mean().item()), float(lv["lnb"].double().mean().item())
        b = f + f"enhance_blocks.{i}.conv_atten."
        lv["ffrm_w"] = sd[b + "conv.weight"].reshape(C, C).contiguous()
        lv["gn_w"], lv["gn_b"] = sd[b + "gn.weight"], sd[b + "gn.bias"]
        b = f + f"detail_feature_extractions.{i}."
        dw = sd[b + "dwconv.weight"]  # [2C, 2, 3, 3], groups=C -> [G=C][tap][ci=2][co=2]
        lv["mlp_in"] = _planes(sd[b + "project_in.weight"].reshape(2 * C, C))
        lv["mlp_dw"] = dw.reshape(C, 2, 2, 9).permute(3, 0, 2, 1).contiguous()   # tap-major [9][g][ci][co]
        lv["mlp_out"] = _planes(sd[b + "project_out.weight"].reshape(C, C))
        lv["s1"], lv["s2"] = scalar(f + f"scale_layers.{i}.scale1"), scalar(f + f"scale_layers.{i}.scale2")
        b = f + f"ca_blocks.{i}.coord_atten."
        mip = max(8, C // 32)
        inv = sd[b + "bn1.weight"] / torch.sqrt(sd[b + "bn1.running_var"] + 1e-5)  # BN(eval) folded into conv1
        w1 = sd[b + "conv1.weight"].reshape(mip, C) * inv[:, None]
        b1 = (sd[b + "conv1.bias"] - sd[b + "bn1.running_mean"]) * inv + sd[b + "bn1.bias"]
        lv["mip"], lv["mip_pad"] = mip, ops.pad32(mip)
        lv["ca1"], lv["ca1_b"] = _planes(w1), b1.contiguous()
        lv["cah"], lv["cah_b"] = _planes(sd[b + "conv_h.weight"].reshape(C, mip)), sd[b + "conv_h.bias"]
        lv["caw"], lv["caw_b"] = _planes(sd[b + "conv_w.weight"].reshape(C, mip)), sd[b + "conv_w.bias"]
        lv["fc"] = _planes(sd[f"spm.fc{i+1}.weight"].reshape(D, C))
        fb = sd[f"spm.fc{i+1}.bias"]
        lv["fc_b"] = (fb + sd["level_embed"][i - 1]).contiguous() if i >= 1 else fb.contiguous()  # BK:149-156 folded
        neck.append(lv)
    return neck


# ---------------------------------------------------------------------------------------------- interactions
def pack_interactions(sd, plan, dev):
    """Injector i normalises the adapter tokens c with its feat_norm, extractor i normalises the SAME c (the injector only updates x) with its query_norm: two LayerNorm passes over the largest
    token matrix of the path (Nc = 21504 rows per image).  LN(c; w, b) W^T + bias = chat (W * w)^T + (W b + bias) with chat = (c - mean) * rstd, so the affine parts are folded into the two
    projections' weights here and ONE pass computes chat for both (`share_c_norm = False` keeps two).  With the adapter-token fold (PackPlan.fold_adapter_ln) the folded projections also carry
    their column sums."""
    cfg, share_c, fold_rn = plan.cfg, plan.share_c_norm, plan.fold_adapter_ln

    def proj(w, bias, index, ln=None, **kw):   # -> (planes, column sums or None, bias) of one projection, `ln` = (lnw, lnb) folded into it
        fmt = plan.inter_fmt(w.shape[1], index, h8c_ok=kw.pop("h8c_ok", True))
        if ln is not None:
            return fold_ln_planes(w, bias, *ln, fmt, f64=False, colsums=fold_rn, **kw)
        if kw.get("pad128"):
            w, bias = _pad_rows128(w, bias)
        return _planes(w, fmt=fmt), None, bias

    def pack_msda(b, index, fold_val=None, fold_oa=None):
        # the offsets + attention-weights projection has 3 * heads * levels * points output columns (192 / 576 at ViT-L): padded with zero rows to whole 128-column GEMM tiles -- the same number of
        # tiles, none of them ragged, so that every tile of the launch takes the register-resident epilogue (a launch that runs both epilogues no longer fits the instruction cache:
        # profiles/r05_epilogue_regs.txt).  The deformable-attention kernel reads the first 3 * heads * levels * points columns of a row (ldraw = the padded width).
        oa, oa_cs, oa_b = proj(torch.cat([sd[b + "sampling_offsets.weight"], sd[b + "attention_weights.weight"]], 0),
                               torch.cat([sd[b + "sampling_offsets.bias"], sd[b + "attention_weights.bias"]], 0), index, fold_oa, pad128=True)
        val, val_cs, val_b = proj(sd[b + "value_proj.weight"], sd[b + "value_proj.bias"], index, fold_val)
        mp = dict(oa=oa, oa_b=oa_b.contiguous(), val=val, val_b=val_b,
                  out=proj(sd[b + "output_proj.weight"], None, index)[0], out_b=sd[b + "output_proj.bias"])
        mp.update((k, v) for k, v in (("oa_cs", oa_cs), ("val_cs", val_cs)) if v is not None)
        return mp

    def pack_extractor(b, index, fold_c=False):
        ep = dict(qnw=sd[b + "query_norm.weight"], qnb=sd[b + "query_norm.bias"], fnw=sd[b + "feat_norm.weight"],
                  fnb=sd[b + "feat_norm.bias"], fold_c=fold_c, first=False, cffn=cfg["with_cffn"],
                  attn=pack_msda(b + "attn.", index, fold_oa=(sd[b + "query_norm.weight"], sd[b + "query_norm.bias"]) if fold_c else None))
        if cfg["with_cffn"]:   # AM:485-488, 499-500
            dw = sd[b + "ffn.dwconv.dwconv.weight"]
            # ffn_norm folded into fc1 (its input is then the un-affine normalised c, or raw c + the row-normalising epilogue)
            fc1, fc1_cs, fc1_b = proj(sd[b + "ffn.fc1.weight"], sd[b + "ffn.fc1.bias"], index, (sd[b + "ffn_norm.weight"], sd[b + "ffn_norm.bias"]) if fold_c else None)
            ep.update(fc1=fc1, fc1_b=fc1_b,
                      dw=dw.reshape(dw.shape[0], 9).t().contiguous(), dw_b=sd[b + "ffn.dwconv.dwconv.bias"],
                      # fc2's A operand is written by the 3 x 3 depthwise conv (mmsa_dwconv_nhwc), which emits bf16 hi/lo and h8 LINE planes only:
                      # a hidden width >= 512 (cffn_ratio 0.5 at embed_dim 1024; the reference's configs stay <= 320) must not pick h8c here
                      fc2=proj(sd[b + "ffn.fc2.weight"], None, index, h8c_ok=False)[0], fc2_b=sd[b + "ffn.fc2.bias"],
                      ffw=sd[b + "ffn_norm.weight"], ffb=sd[b + "ffn_norm.bias"])
            if fc1_cs is not None:
                ep["fc1_cs"] = fc1_cs
        return ep

    inter = []
    idxs = cfg["interaction_indexes"]
    for i in range(len(idxs)):
        b = f"interactions.{i}."
        it = dict(inj=dict(gamma=sd[b + "injector.gamma"], qnw=sd[b + "injector.query_norm.weight"],
                           qnb=sd[b + "injector.query_norm.bias"], fnw=sd[b + "injector.feat_norm.weight"],
                           fnb=sd[b + "injector.feat_norm.bias"], fold_c=share_c,
                           attn=pack_msda(b + "injector.attn.", i, fold_val=(sd[b + "injector.feat_norm.weight"], sd[b + "injector.feat_norm.bias"]) if share_c else None)),
                  ext=[pack_extractor(b + "extractor.", i, fold_c=share_c)])
        it["ext"][0]["first"] = True     # the extractor that shares the injector's un-affine normalised c (share_c_norm) when nothing is folded further
        if i == len(idxs) - 1 and cfg["use_extra_extractor"]:   # BK:91-92
            it["ext"] += [pack_extractor(b + "extra_extractors.0.", i, fold_c=share_c), pack_extractor(b + "extra_extractors.1.", i, fold_c=share_c)]
        it["inj"]["first_block"] = idxs[i][0]   # whose qkv GEMM reads the stream planes the injector writes (LayerNorm fold)
        inter.append(it)
    return inter


def pack_tail(sd, plan, dev):
    D = plan.D
    up = sd["up.weight"]   # ConvTranspose2d(D,D,2,2) weight [Cin, Cout, 2, 2] -> rows (i,j,co), K = ci  (BK:55,324)
    bn = []
    for i in range(1, 5):
        inv = sd[f"norm{i}.weight"] / torch.sqrt(sd[f"norm{i}.running_var"] + 1e-5)
        bn.append((inv.contiguous(), (sd[f"norm{i}.bias"] - sd[f"norm{i}.running_mean"] * inv).contiguous()))
    return dict(up=_planes(up.permute(2, 3, 1, 0).reshape(4 * D, D), fmt=plan.inter_fmt(D, site="up")), up_b=sd["up.bias"].repeat(4).contiguous(),
                bn=bn, pos_src=sd["pos_embed"])


@torch.no_grad()
def pack(model, dev):
    """Pre-pack `model`'s weights for `dev`.  The guard words of the model live here too: one logit word per ViT block (check_attention_guard) and, last,
    the clamp watch word (include/mmsa.h "Clamp watch") -- weight planes that had to clamp a value report into it like every forward's activations do."""
    plan = PackPlan.of(model)
    depth = plan.cfg["depth"]
    guard = torch.zeros(depth + 1, device=dev)
    carry, model._carry_modes = getattr(model, "_carry_modes", None), None
    with ops.clamp_watch(guard[depth:]):
        sd = float_state_dict(model, dev)
        pk = {"h8_sites": plan.h8_sites, "h8c": plan.h8c}
        pk.update(pack_vit(sd, plan, dev))
        pk.update(cnx_f16=plan.cnx_f16, fold_cnx_ln=plan.fold_cnx_ln, twin2=pack_twin(sd, plan, dev), neck=pack_neck(sd, plan, dev),
                  share_c_norm=plan.share_c_norm, ln_one=torch.ones(plan.D, device=dev), ln_zero=torch.zeros(plan.D, device=dev),
                  fold_adapter_ln=plan.fold_adapter_ln, inter=pack_interactions(sd, plan, dev))
        pk.update(pack_tail(sd, plan, dev))
        pk["geom"] = {}
        torch.cuda.synchronize(dev)
        if carry is not None and len(carry) == len(pk["blocks"]):
            # a pack was dropped whose blocks had settled their attention precision (the switch to the wide-range state; interactions following their blocks): the decisions carry over
            modes = [dict(max_logit=ml, **({} if amode is None else {"amode": amode})) for amode, ml in carry]
            carry_block_modes(pk, modes, lambda: sd, plan, dev)
    pk["attn_guard"] = guard
    # a WEIGHT that had to be clamped stays clamped in its planes: kept as a host-side flag of this pack (the device word is zeroed with every
    # refusal, the planes are not repacked by that: ADVICE r05) -- check_attention_guard() goes wide / refuses on it until the pack is dropped
    pk["weights_clamped"] = float(guard[depth].item())
    guard[depth:].zero_()
    pk["wide"] = plan.wide
    pk["inter_pairs"] = sorted(plan.inter_pairs)
    return pk
