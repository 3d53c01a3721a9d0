#!/usr/bin/env python3
"""Percentile5 on long rows: the register-resident kernel at 4096 x 16384 float32 (for
scale) and the radix-select kernel of percentile_long.h at 4096 x 32768 and 2048 x 65536
float32 and 2048 x 32768 complex64 (|standard normal| and circular complex noise). Every
configuration is timed with device events after a warm-up, the configurations alternating
within each round; the figure is the median over rounds. Each timed output is checked
against the CPU oracle on two slices of rows.
usage: tools/time_percentile_long.py [rounds]"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from katsdpsigproc_amd import accel, percentile  # noqa: E402
from oracle import rfi_oracle as oracle  # noqa: E402

SHAPES = ((4096, 16384, True), (4096, 32768, True), (2048, 65536, True), (2048, 32768, False))
CALLS = 5
CHECK = 8  # rows per checked slice
HBM = 8e12  # bytes/s


def main() -> None:
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 7
    ctx = accel.create_some_context(False)
    q = ctx.create_command_queue()
    rng = np.random.default_rng(61)
    oracle.set_threads(min(oracle.max_threads(), 16))

    ops = []  # (rows, cols, is_amplitude, operation, check)
    for r, c, amp in SHAPES:
        if amp:
            ary = np.abs(rng.standard_normal((r, c), dtype=np.float32))
        else:
            ary = rng.standard_normal((r, 2 * c), dtype=np.float32).view(np.complex64)
        op = percentile.Percentile5Template(ctx, c, is_amplitude=amp).instantiate(q, (r, c))
        op.ensure_all_bound()
        op.buffer("src").set(q, ary)

        def check(op, ary=ary, r=r):
            out = op.buffer("dest").get(q)
            ok = True
            for sl in (slice(0, CHECK), slice(r - CHECK, r)):
                ok &= np.array_equal(oracle.percentile5(ary[sl]), out[:, sl])
            return ok

        ops.append((r, c, amp, op, check))
        del ary

    for _, _, _, op, _ in ops:  # warm-up: code objects loaded, clocks up
        for _ in range(5):
            op()
    q.finish()
    times = {i: [] for i in range(len(ops))}
    for _ in range(rounds):
        for i, (_, _, _, op, _) in enumerate(ops):
            a = q.enqueue_marker()
            for _ in range(CALLS):
                op()
            e = q.enqueue_marker()
            q.finish()
            times[i].append(1e3 * e.time_since(a) / CALLS)

    print(f"# {ctx.device.name}: {rounds} rounds x {CALLS} calls per configuration, "
          f"alternating; median (min) ms per call")
    ok_all = True
    per_elem = {}
    for i, (r, c, amp, op, check) in enumerate(ops):
        ts = np.array(times[i])
        ms = float(np.median(ts))
        ok = check(op)
        ok_all &= ok
        per_elem[(c, amp)] = ms / (r * c)
        nbytes = (4 if amp else 8) * r * c
        gbs = nbytes / (ms * 1e6)
        kind = "float32" if amp else "complex64"
        print(f"{kind:9s} {r:5d} x {c:6d}  {ms:8.4f} ms ({ts.min():8.4f})  {gbs:7.0f} GB/s "
              f"({gbs * 1e9 / HBM:5.1%} of 8 TB/s)  oracle slices: {'match' if ok else 'MISMATCH'}")
    ratio = per_elem[(32768, True)] / per_elem[(16384, True)]
    print(f"per-element time, float32 4096 x 32768 / 4096 x 16384 = {ratio:.2f}")
    if not ok_all:
        sys.exit(1)


if __name__ == "__main__":
    main()
