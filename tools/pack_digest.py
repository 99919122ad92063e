"""One sha1 per packed tree: what `model._pack(dev)` returns, hashed in traversal order -- dict keys, every tensor's shape, dtype and bytes, the
buffer / n / k / kpad / fmt / weight / split of every Planes (the stacked buffer where there is one), repr() of every other leaf.  Pack only, no
forward.  The script uses what every revision since the packed format 12 has (mmsa.build_backbone, tests.weights, model._pack, attribute
assignment), so it runs unchanged in a checkout of another commit: equal digests = the two revisions pack the same tree, byte for byte.

  python tools/pack_digest.py [--out FILE]                 the digest table (+ the wall time of the default ViT-L pack)
  python tools/pack_digest.py --save FILE                  tiny256 with peaky attention, one eager forward, checkpoint.save_packed -> FILE
  python tools/pack_digest.py --load FILE                  load FILE into a fresh model (load_packed must not repack), one forward, digest of the outputs

(checkpoint._packed_checksum skips the non-tensor leaves and the Planes' attributes: hence the walker here.)"""
import argparse
import hashlib
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "multimodal-sam-adapter_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

import mmsa  # noqa: E402
from mmsa import ops  # noqa: E402
from tests.configs import CONFIGS, make_input  # noqa: E402
from tests.weights import peaky_attention, seeded_state_dict  # noqa: E402

DEFAULT_CASES = ("tiny256", "tiny256_plain", "tiny256_norel", "hd80_256", "vitb512", "vitl1024", "vith1024", "vitl800")
H8_DEFAULT = ("vit", "inter", "up", "attnv")
# each alone, on tiny256 and on vitl1024
VARIANTS = [("h8_sites=()", dict(h8_sites=())), ("h8_sites+cnx,cnx2,cnx2p2", dict(h8_sites=H8_DEFAULT + ("cnx", "cnx2", "cnx2p2"))),
            ("h8c=False", dict(h8c=False)), ("cnx_f16=False", dict(cnx_f16=False)), ("fold_ln=False", dict(fold_ln=False)),
            ("share_c_norm=False", dict(share_c_norm=False)), ("fold_adapter_ln=True", dict(fold_adapter_ln=True)),
            ("fold_convnext_ln=True", dict(fold_convnext_ln=True)), ("fuse_gfe_qkv=False", dict(fuse_gfe_qkv=False)),
            ("_wide_range=True", dict(_wide_range=True)), ("_inter_pairs={1}", dict(_inter_pairs={1})), ("_carry_modes[1]=b3", "carry"),
            ("fp8_weights=True", dict(fp8_weights=True))]


def _tensor(h, t):
    t = t.detach().contiguous().cpu()
    h.update(repr((tuple(t.shape), str(t.dtype))).encode())
    h.update(t.reshape(-1).view(torch.uint8).numpy().tobytes())


def _walk(h, o):
    if isinstance(o, ops.Planes):
        full = getattr(o, "full", None)
        h.update(b"<planes>")
        _tensor(h, full if full is not None else o.p)
        h.update(repr((o.n, o.k, o.kpad, o.fmt, o.weight, o.split, full is not None)).encode())
    elif isinstance(o, torch.Tensor):
        _tensor(h, o)
    elif isinstance(o, dict):
        h.update(b"<dict>")
        for k, v in o.items():
            h.update(repr(k).encode())
            _walk(h, v)
    elif isinstance(o, (list, tuple)):
        h.update(f"<{type(o).__name__} {len(o)}>".encode())
        for v in o:
            _walk(h, v)
    else:
        h.update(repr(o).encode())


def tree_digest(tree):
    h = hashlib.sha1()
    _walk(h, tree)
    return h.hexdigest()


def build(name):
    cfg = CONFIGS[name]
    m = mmsa.build_backbone(dict(type=cfg.get("type", "SAMAdapterbimodalMixModNewInTwinConvNEW"), **cfg["kwargs"]))
    m.load_state_dict(seeded_state_dict(m, seed=cfg["seed"]), strict=True)
    return m


def pack_case(m, attrs, dev):
    """Digest of one pack of `m` with `attrs` set (then removed again, the model invalidated), or the text of the ValueError it raised."""
    m.invalidate()
    if attrs == "carry":
        attrs = dict(_carry_modes=[("b3", 9.5) if i == 1 else (None, 0.0) for i in range(m.cfg["depth"])])
    for k, v in attrs.items():
        setattr(m, k, v)
    try:
        with torch.cuda.device(dev):
            t0 = time.perf_counter()
            pk = m._pack(dev)
            torch.cuda.synchronize(dev)
            dt = time.perf_counter() - t0
        return tree_digest(pk), dt
    except ValueError as e:
        return "ValueError: " + str(e), 0.0
    finally:
        for k in attrs:
            if k in m.__dict__:
                delattr(m, k)
        m.invalidate()


def table(out):
    dev = torch.device("cuda", 0)
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)
    for name in DEFAULT_CASES:
        m = build(name)
        d, dt = pack_case(m, {}, dev)
        emit(f"{name:<12} {'default':<28} {d}")
        if name == "vitl1024":
            d2, dt2 = pack_case(m, {}, dev)    # (the first pack of a process also pays for loading the code objects)
            assert d2 == d
            emit(f"# vitl1024 default pack wall time: first {dt:.2f} s, again {dt2:.2f} s")
        if name in ("tiny256", "vitl1024"):
            for label, attrs in VARIANTS:
                emit(f"{name:<12} {label:<28} {pack_case(m, attrs, dev)[0]}")
        del m
    if out:
        with open(out, "w") as f:
            f.write("\n".join(lines) + "\n")


def _peaky_tiny():
    cfg = CONFIGS["tiny256"]
    m = mmsa.build_backbone(dict(type="SAMAdapterbimodalMixModNewInTwinConvNEW", **cfg["kwargs"]))
    m.load_state_dict(peaky_attention(seeded_state_dict(m, seed=cfg["seed"]), cfg["kwargs"]["embed_dim"], 4.0), strict=True)
    return m, make_input(cfg, batch=2).to("cuda:0")


def save(path):
    from mmsa.checkpoint import save_packed
    m, x = _peaky_tiny()
    m(x)
    torch.cuda.synchronize()
    print("modes", [a for a, _ in m.attention_modes()], "inter_pairs", sorted(m._inter_pairs))
    save_packed(m, path, device="cuda:0")
    blob = torch.load(path, map_location="cpu")
    for k in ("settings", "packed_checksum", "fingerprint"):
        v = blob[k]
        print(k, v if k != "fingerprint" else v[1])
    print("file_tree", tree_digest(blob["packed"]))


def load(path):
    from mmsa.checkpoint import load_packed
    x = make_input(CONFIGS["tiny256"], batch=2).to("cuda:0")

    def boom(dev):
        raise AssertionError("load_packed repacked")
    m2 = mmsa.build_backbone(dict(type="SAMAdapterbimodalMixModNewInTwinConvNEW", **CONFIGS["tiny256"]["kwargs"]))
    load_packed(m2, path, device="cuda:0")
    m2._pack = boom
    outs, _ = m2(x)
    torch.cuda.synchronize()
    print("loaded", path, "modes", [a for a, _ in m2.attention_modes()], "outputs", tree_digest([o for o in outs]))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--save")
    ap.add_argument("--load")
    a = ap.parse_args()
    if a.save:
        save(a.save)
    elif a.load:
        load(a.load)
    else:
        table(a.out)
