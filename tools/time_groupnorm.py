"""Isolated device-event timings of GroupNorm32 (+SiLU) forward and backward (bf16, frozen, with accum) at the production shapes
of the SD1.5 training step (B = 8): the forms cl_debug_groupnorm_group(0) leaves (gn1_* / two launches) against the form with
one workgroup per (sample, group) (csrc/norm.hip gng_*), mode 1 = by rule, and -- with --naive -- mode 5, the same kernel with
workgroup ids mapped to (sample, group) pairs in plain order.  --force times mode 2 / 6 (whenever the slab fits) instead, to
measure classes the rule leaves out.

All modes run interleaved in one process.  A figure is microseconds per call over a window of --iters back-to-back launches
between two events; a group is the median of --rounds such windows per mode; --groups groups are taken.  Reported per shape,
direction and mode: the median of the group medians, and their range (max - min): the range of mode 0 is the spread a gain
has to exceed.  Two cache regimes: "same" relaunches on one set of buffers (a 21 - 63 MB working set stays in the 256 MiB
Infinity Cache, as a tensor a neighbouring kernel has just written does in the step), "rotating" walks over enough buffer
sets that every launch reads from HBM.

    python tools/time_groupnorm.py [--out profiles/gn_group/time_groupnorm.json] [--naive] [--force]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ctrlora_amd import hip  # noqa: E402

B, G = 8, 32
SHAPES = [(4096, 320), (4096, 640), (4096, 960), (1024, 320), (1024, 640), (1024, 960), (1024, 1280), (1024, 1920),
          (256, 640), (256, 1280), (256, 1920), (256, 2560)]
FORMS = {1: "gn1", 2: "two-launch", 3: "three-launch", 4: "coop", 5: "group"}


def probe():
    out = (ctypes.c_int * 12)()
    assert hip.lib().cl_debug_norm_last_launch(out) == 0
    return list(out)


class Buffers:
    def __init__(self, HW, C, sets):
        g = torch.Generator(device="cuda").manual_seed(HW + C)
        mk = lambda: (torch.randn(B * HW, C, device="cuda", generator=g) * 1.5 + 0.3).bfloat16()
        self.HW, self.C = HW, C
        self.sets = [dict(x=mk(), dy=mk(), acc=mk(), y=torch.empty(B * HW, C, device="cuda", dtype=torch.bfloat16),
                          dx=torch.empty(B * HW, C, device="cuda", dtype=torch.bfloat16)) for _ in range(sets)]
        self.gamma = 1 + 0.2 * torch.randn(C, device="cuda", generator=g)
        self.beta = 0.2 * torch.randn(C, device="cuda", generator=g)
        self.stats = torch.empty(B, G, 2, device="cuda")
        self.ws = torch.empty(hip.groupnorm_ws(B, HW, C), device="cuda")

    def fwd(self, i):
        s = self.sets[i % len(self.sets)]
        hip.groupnorm_fwd(s["x"], s["y"], self.gamma, self.beta, B, self.HW, 1e-5, True, self.stats, self.ws)

    def bwd(self, i):
        s = self.sets[i % len(self.sets)]
        hip.groupnorm_bwd(s["x"], s["dy"], s["dx"], self.gamma, self.beta, self.stats, B, self.HW, True, self.ws, accum=s["acc"])


def window(call, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for i in range(iters):
        call(i)
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / iters


def measure(buf, direction, modes, a):
    L = hip.lib()
    call = buf.fwd if direction == "fwd" else buf.bwd
    forms, meds = {}, {m: [] for m in modes}
    for m in modes:                                    # warm-up of every mode; the statistics the backward reads come from here
        assert L.cl_debug_groupnorm_group(m) == 0
        for i in range(len(buf.sets) + 2):
            buf.fwd(i)
            call(i)
        forms[m] = probe()
    torch.cuda.synchronize()
    for _ in range(a.groups):
        t = {m: [] for m in modes}
        for _ in range(a.rounds):
            for m in modes:
                L.cl_debug_groupnorm_group(m)
                t[m].append(window(call, a.iters))
        for m in modes:
            meds[m].append(statistics.median(t[m]))
    L.cl_debug_groupnorm_group(1)
    return {m: dict(form=FORMS.get(forms[m][1], forms[m][1]), nv=forms[m][3], threads=forms[m][5], grid=forms[m][8] * forms[m][9],
                    us=statistics.median(meds[m]), range_us=max(meds[m]) - min(meds[m]), group_medians_us=meds[m]) for m in modes}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "gn_group", "time_groupnorm.json"))
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--groups", type=int, default=5)
    ap.add_argument("--naive", action="store_true")
    ap.add_argument("--force", action="store_true")
    ap.add_argument("--shapes", default="", help="comma-separated HWxC, default: all production shapes")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_groupnorm: needs a GPU")
    new = 2 if a.force else 1
    modes = [0, new] + ([new + 4] if a.naive else [])
    shapes = [tuple(int(v) for v in s.split("x")) for s in a.shapes.split(",")] if a.shapes else SHAPES
    rows = []
    for HW, C in shapes:
        per_set = B * HW * C * 2 * 5
        for regime, sets in (("same", 1), ("rotating", max(2, -(-(640 << 20) // per_set)))):
            buf = Buffers(HW, C, sets)
            for direction in ("fwd", "bwd"):
                r = measure(buf, direction, modes, a)
                old, cur = r[0], r[new]
                row = dict(HW=HW, C=C, direction=direction, cache=regime, sets=sets, old=old, new=cur,
                           gain_us=old["us"] - cur["us"], beats_spread=bool(old["us"] - cur["us"] > old["range_us"]))
                if a.naive:
                    row["new_naive_ids"] = r[new + 4]
                rows.append(row)
                print(f"{HW:5d} x {C:4d} {direction} {regime:8s} old {old['form']:>10s} {old['us']:7.2f} us (range {old['range_us']:.2f})"
                      f"  new {cur['form']:>10s} {cur['us']:7.2f} us" + (f"  naive ids {r[new + 4]['us']:7.2f} us" if a.naive else "")
                      + f"  gain {row['gain_us']:6.2f} us  beats spread: {row['beats_spread']}", flush=True)
            del buf
            torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(dict(device=torch.cuda.get_device_name(0), B=B, G=G, iters=a.iters, rounds=a.rounds, groups=a.groups, forced=a.force,
                       rows=rows), f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
