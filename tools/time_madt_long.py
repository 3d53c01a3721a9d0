#!/usr/bin/env python3
"""NoiseEstMADT on long bands: the baseline-major noise estimate alone at 16384 x 8192
(the register-resident kernel, for scale), 32768 x 4096, 65536 x 2048 and 262144 x 512
(the radix-select kernel of madnz_long.h; 512 MiB of float32 each, standard normal with
10 % zeros), and the kernel-per-stage flagger (width 13, SumThreshold with 4 windows,
11 sigma) on 32768 channels x 4096 baselines of complex noise with interference on 1/16
of the samples. Every configuration is timed with device events after a warm-up, the
configurations alternating within each round; the figure is the median over rounds.
Each timed output is checked against the CPU oracle on two slices of baselines.
usage: tools/time_madt_long.py [rounds]"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from katsdpsigproc_amd import accel  # noqa: E402
from katsdpsigproc_amd.rfi import device  # noqa: E402
from oracle import rfi_oracle as oracle  # noqa: E402
from tests import inputs  # noqa: E402

MADT_SHAPES = ((16384, 8192), (32768, 4096), (65536, 2048), (262144, 512))
SEQ_SHAPE = (32768, 4096)
CALLS = 5
CHECK = 8  # baselines per checked slice


def main() -> None:
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 7
    ctx = accel.create_some_context(False)
    q = ctx.create_command_queue()
    rng = np.random.default_rng(51)
    oracle.set_threads(min(oracle.max_threads(), 16))

    ops = []  # (name, channels, baselines, operation, check)
    for c, b in MADT_SHAPES:
        dev = rng.standard_normal((b, c), dtype=np.float32)
        dev[rng.random((b, c), dtype=np.float32) < 0.1] = 0.0
        op = device.NoiseEstMADTDeviceTemplate(ctx, c).instantiate(q, c, b)
        op.ensure_all_bound()
        op.buffer("deviations").set(q, dev)

        def check(op, dev=dev, b=b):
            out = op.buffer("noise").get(q)
            ok = True
            for sl in (slice(0, CHECK), slice(b - CHECK, b)):
                ref = oracle.NoiseEstMADHost()(np.ascontiguousarray(dev[sl].T)).astype(np.float32)
                ok &= np.array_equal(ref, out[sl])
            return ok

        ops.append(("madt", c, b, op, check))
        del dev

    c, b = SEQ_SHAPE
    vis_host = inputs.add_rfi(inputs.generate_data(c, b, seed=52), seed=53)
    t = device.FlaggerDeviceTemplate(
        device.BackgroundMedianFilterDeviceTemplate(ctx, 13, tuning={"wgs": 64, "csplit": 0}),
        device.NoiseEstMADTDeviceTemplate(ctx, c),
        device.ThresholdSumDeviceTemplate(ctx, 4, tuning={"wgsx": 256, "vt": 0}),
        fused=False)
    op = t.instantiate(q, c, b, threshold_args={"n_sigma": 11.0})
    assert isinstance(op, device.FlaggerDevice)
    op.ensure_all_bound()
    op.buffer("vis").set(q, vis_host)

    def check_seq(op):
        noise, flags = op.buffer("noise").get(q), op.buffer("flags").get(q)
        ok = True
        for sl in (slice(0, CHECK), slice(b - CHECK, b)):
            v = np.ascontiguousarray(vis_host[:, sl])
            dev32 = oracle.BackgroundMedianFilterHost(13)(v).astype(np.float32)
            noise32 = oracle.NoiseEstMADHost()(dev32).astype(np.float32)
            ok &= np.array_equal(noise32, noise[sl])
            ok &= np.array_equal(oracle.ThresholdSumHost(11.0, 4)(dev32, noise32), flags[:, sl])
        return ok

    ops.append(("sequence", c, b, op, check_seq))

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
    per_sample = {}
    for i, (kind, c, b, op, check) in enumerate(ops):
        ts = np.array(times[i])
        ms = float(np.median(ts))
        ok = check(op)
        ok_all &= ok
        per_sample[(kind, c)] = ms / (c * b)
        rate = (f"{4 * c * b / (ms * 1e6):7.0f} GB/s" if kind == "madt"
                else f"{c * b / (ms * 1e-3):.3e} samples/s")
        print(f"{kind:8s} {c:6d} x {b:5d}  {ms:8.4f} ms ({ts.min():8.4f})  {rate}  "
              f"oracle slices: {'match' if ok else 'MISMATCH'}")
    ratio = per_sample[("madt", 32768)] / per_sample[("madt", 16384)]
    print(f"per-sample time, 32768 x 4096 / 16384 x 8192 = {ratio:.2f} (yardstick: at most 2)")
    if not ok_all:
        sys.exit(1)


if __name__ == "__main__":
    main()
