"""Timing of the run-length tables for profiles/run_length.txt.  Legs interleaved in ONE process, every repetition timing each leg once (order rotated),
`--inner` calls per timing between two events on the launch stream, all on the same stored maps and into given tables:
  (cr) / (cc)    mmsa_run_lengths_u8 of the class map, row order / column order (the library's transpose into the table's scratch, then the row launches);
  (ir) / (ic)    mmsa_run_lengths_i32 of the `ids` of the class map's SegmentTable, row / column;
  (tc) / (ti)    the column order from outside: map.transpose(1, 2) copied by torch into a given buffer, then the ROW-order launch on it -- class map / ids;
  (dec)          mmsa_run_decode_i32 of the column table of ids;
  (upd) / (updr) the full SegmentTable.update() without runs / with runs="column";
  (noi) / (one)  the worst cases, column order: a 25-class noise map at capacity = H * W (almost every pixel a run) and the one-value map (one run);
  yardsticks on the same maps: (tab) mmsa_segment_table with roots given (the same scan structure), (e) mmsa_eval_confusion_u8 (the launch floor);
  (host)         the host route, timed with the wall clock (3 repetitions): copy `ids` to the host, then the numpy restatement of the column runs.
Before anything is timed every device table of image 0 is checked against the numpy restatement on the full-size map, (tc) / (ti) against (cc) / (ic)
byte for byte, and the decoded table against ids.
The rule the column order was chosen by: a form of its own stays only if (cc) beats (tc) and (ic) beats (ti) by more than the p10 .. p90 span of (tc) / (ti)
on both workloads; the last line of every workload gives both differences.  The LDS-tiled column walk that was built first did not (its report is kept in
profiles/run_length.txt), so (cc) / (ic) are now the same route as (tc) / (ti) with the library's own transpose kernel.
Workloads, 25 classes, as tools/exp/segment_table_bench.py: two 1024 x 1024 maps and the 1080 x 1920 frame.  The medians and p10 .. p90 are the record."""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "multimodal-sam-adapter_amd"))
sys.path.insert(0, ROOT)


def numpy_runs(m, order):
    """The restatement: one image [H, W] -> (starts, values) of every run."""
    flat = (m if order == "row" else m.T).ravel()
    starts = np.flatnonzero(np.r_[True, flat[1:] != flat[:-1]])
    return starts, flat[starts].astype(np.int64)


def check(table, m):
    """The table of image 0 against the restatement on the full-size map -> the number of runs."""
    starts, values = numpy_runs(m, table.order)
    n = int(table.count[0])
    assert n == len(starts) <= table.capacity, f"{n} runs, the restatement has {len(starts)}, capacity {table.capacity}"
    assert np.array_equal(table.starts[0, :n].cpu().numpy(), starts) and np.array_equal(table.values[0, :n].cpu().numpy(), values), table.order
    return n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--inner", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--tag", default="", help="a line for the head of the report: which build this is")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("run_length_bench: no GPU (a timing needs one)")
    import mmsa
    import mmsa.inference as inf
    from mmsa import evaluate as E
    from mmsa.evaluate import LabelPrep, RunTable, SegmentTable
    import torch.nn.functional as F
    dev = torch.device("cuda", 0)
    lines = []
    C = 25

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    def logits(n, g):
        coarse = torch.randn(n, C, 32, 32, generator=g)
        return (F.interpolate(coarse, size=(256, 256), mode="bilinear") + 0.05 * torch.randn(n, C, 256, 256, generator=g)).to(dev)

    say(f"device {torch.cuda.get_device_name(0)}; reps {a.reps}, {a.inner} calls per timing; times in microseconds per call; {C} classes; scan block "
        f"{E.RUNS_BLOCK} pixels, transpose tile {E.RUNS_TILE} x {E.RUNS_TILE}, {E.SCAN_TRIP} unit counts per scan trip" + (f"; {a.tag}" if a.tag else ""))
    g = torch.Generator().manual_seed(7)
    lp = LabelPrep(C)
    for name, plan in (("two 1024 x 1024 maps", inf.MapPlan.whole(2, 1024, 1024)),
                       ("1080 x 1920 frame, six windows", inf.MapPlan.slide(1, 1080, 1920, (1024, 1024), (640, 640)))):
        lg = logits(plan.n, g)
        B, H, W = plan.B, plan.Ho, plan.Wo
        pred = torch.empty(B, H, W, dtype=torch.uint8, device=dev)
        unc = torch.zeros(1, dtype=torch.int32, device=dev)
        plan.class_map(lg, pred, unc)
        assert int(unc.item()) == 0
        del lg
        lab = torch.roll(pred, (3, 2), (1, 2)).contiguous()
        noise = torch.randint(0, C, (B, H, W), generator=g, dtype=torch.uint8).to(dev)
        one = torch.full((B, H, W), 7, dtype=torch.uint8, device=dev)
        root = mmsa.components(pred, num_classes=C)
        st, st_upd, st_runs = SegmentTable(num_classes=C), SegmentTable(num_classes=C), SegmentTable(num_classes=C, runs="column")
        st.update(pred, root=root)
        st_upd.update(pred), st_runs.update(pred)
        ids = st.ids
        assert not st.overflow() and torch.equal(st_runs.ids, ids)
        cap = E.default_run_capacity(H, W)
        t = {k: RunTable.empty(B, H, W, o, cap, dev) for k, o in (("cr", "row"), ("cc", "column"), ("ir", "row"), ("ic", "column"), ("one", "column"))}
        t["noi"] = RunTable.empty(B, H, W, "column", H * W, dev)
        t["tc"], t["ti"] = RunTable.empty(B, W, H, "row", cap, dev), RunTable.empty(B, W, H, "row", cap, dev)      # the transposed maps, row order
        pred_t, ids_t = torch.empty(B, W, H, dtype=torch.uint8, device=dev), torch.empty(B, W, H, dtype=torch.int32, device=dev)
        dec = torch.empty(B, H, W, dtype=torch.int32, device=dev)
        ebuf = torch.zeros(B, C + 1, C + 1, dtype=torch.int64, device=dev)

        def transposed(src, dst, table):
            dst.copy_(src.transpose(1, 2))
            mmsa.run_lengths(dst, table=table)

        legs = dict(
            cr=lambda: mmsa.run_lengths(pred, table=t["cr"]), cc=lambda: mmsa.run_lengths(pred, table=t["cc"]),
            ir=lambda: mmsa.run_lengths(ids, table=t["ir"]), ic=lambda: mmsa.run_lengths(ids, table=t["ic"]),
            tc=lambda: transposed(pred, pred_t, t["tc"]), ti=lambda: transposed(ids, ids_t, t["ti"]),
            dec=lambda: mmsa.run_decode(t["ic"], out=dec),
            upd=lambda: st_upd.update(pred), updr=lambda: st_runs.update(pred),
            noi=lambda: mmsa.run_lengths(noise, table=t["noi"]), one=lambda: mmsa.run_lengths(one, table=t["one"]),
            tab=lambda: st.update(pred, root=root), e=lambda: mmsa.confusion(pred, lab, lp, counts=ebuf))
        what = dict(cr="mmsa_run_lengths_u8, class map, row order", cc="mmsa_run_lengths_u8, class map, column order",
                    ir="mmsa_run_lengths_i32, ids, row order", ic="mmsa_run_lengths_i32, ids, column order",
                    tc="class map: torch's transpose into a given buffer + the row-order launch (yardstick of (cc))",
                    ti="ids: torch's transpose into a given buffer + the row-order launch (yardstick of (ic))",
                    dec="mmsa_run_decode_i32 of the column table of ids", upd="SegmentTable.update() without runs: components + the table",
                    updr="SegmentTable.update() with runs='column'", noi="column runs of a 25-class noise map at capacity = H * W",
                    one="column runs of a one-value map: one run", tab="mmsa_segment_table, roots given, no values (yardstick: the same scan structure)",
                    e="mmsa_eval_confusion_u8 (the floor)")
        for k in legs:
            legs[k]()
        torch.cuda.synchronize()
        host_pred, host_ids = pred[0].cpu().numpy(), ids[0].cpu().numpy()
        n = {k: check(t[k], m) for k, m in (("cr", host_pred), ("cc", host_pred), ("ir", host_ids), ("ic", host_ids), ("noi", noise[0].cpu().numpy()))}
        assert check(st_runs.runs, host_ids) == n["ic"] and t["one"].count.cpu().tolist() == [1] * B
        for alt, own in (("tc", "cc"), ("ti", "ic")):      # the alternative makes the same table
            assert all(torch.equal(getattr(t[alt], f), getattr(t[own], f)) for f in ("count",)) and torch.equal(t[alt].starts[0, :n[own]], t[own].starts[0, :n[own]])
            assert torch.equal(t[alt].values[0, :n[own]], t[own].values[0, :n[own]])
        assert torch.equal(dec, ids) and not any(t[k].overflow() for k in t)
        counts = {k: t[k].count.cpu().tolist() for k in ("cr", "cc", "ir", "ic", "noi")}
        times = {k: [] for k in legs}
        order = list(legs)
        for rep in range(a.reps):
            for k in order[rep % len(order):] + order[:rep % len(order)]:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.inner):
                    legs[k]()
                e1.record()
                e1.synchronize()
                times[k].append(e0.elapsed_time(e1) * 1e3 / a.inner)
        say()
        say(f"{name}: {B * H * W} pixels; the tables of image 0 equal the numpy restatement on the full-size map, the transposed route makes the same tables and "
            f"run_decode gives ids back; runs per image: class map {counts['cr']} row / {counts['cc']} column, ids {counts['ir']} row / {counts['ic']} column at "
            f"capacity {cap}, noise map {counts['noi']} at capacity {H * W}")
        med, span = {}, {}
        for k in legs:
            v = np.array(times[k])
            med[k], span[k] = float(np.median(v)), float(np.percentile(v, 90) - np.percentile(v, 10))
            say(f"  ({k:4s}) {what[k]:100s} median {med[k]:10.2f}   p10 {np.percentile(v, 10):10.2f}   p90 {np.percentile(v, 90):10.2f}")
        say(f"  runs add (updr) - (upd) = {med['updr'] - med['upd']:.2f}; (cc) / (tab) = {med['cc'] / med['tab']:.2f} x, (cc) / (e) = {med['cc'] / med['e']:.2f} x; "
            f"(tc) - (cc) = {med['tc'] - med['cc']:.2f} against a p10 .. p90 span of (tc) of {span['tc']:.2f}; (ti) - (ic) = {med['ti'] - med['ic']:.2f} against "
            f"{span['ti']:.2f}; the transpose costs (cc) - (cr) = {med['cc'] - med['cr']:.2f}, (ic) - (ir) = {med['ic'] - med['ir']:.2f}")
        ts = []
        for _ in range(3):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            nh = sum(len(numpy_runs(m, "column")[0]) for m in ids.cpu().numpy())
            ts.append((time.perf_counter() - t0) * 1e3)
        say(f"  (host) copy of ids + the numpy restatement of the column runs: {nh} runs, {min(ts):.1f} .. {max(ts):.1f} ms per batch (wall clock, 3 repetitions), "
            f"{np.median(ts) * 1e3 / med['ic']:.0f} x (ic)")
        del pred, lab, noise, one, root, st, st_upd, st_runs, ids, t, pred_t, ids_t, dec
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
