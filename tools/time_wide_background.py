#!/usr/bin/env python3
"""Wide median windows: the standalone background operation at widths 31 (the narrow
kernel, for scale), 33, 63, 127 and 255, and the kernel-per-stage flagger at 33 and 255,
on 4096 channels x 8192 baselines of complex noise with sparse interference; without
input flags and with 1/16 per-sample flags. Every configuration is timed with device
events after a warm-up, the configurations alternating within each round; the figure is
the median over rounds. Each timed output is checked against the CPU oracle on two
slices of 32 baselines (deviations bit for bit; the flagger's noise and flags as well).
The launcher picks the channel split (csplit 0) for every width.
usage: tools/time_wide_background.py [rounds]"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from katsdpsigproc_amd import accel  # noqa: E402
from katsdpsigproc_amd.rfi import device  # noqa: E402
from oracle import rfi_oracle as oracle  # noqa: E402
from tests import inputs  # noqa: E402

C, B = 4096, 8192
WIDTHS = (31, 33, 63, 127, 255)
SEQ_WIDTHS = (33, 255)
CALLS = 10
SLICES = (slice(0, 32), slice(B - 32, B))


def main() -> None:
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 7
    ctx = accel.create_some_context(False)
    q = ctx.create_command_queue()
    vis_host = inputs.add_rfi_sparse(inputs.generate_data(C, B, seed=41), seed=42)
    flags_host = (np.random.RandomState(43).random_sample((C, B)) < 1 / 16).astype(np.uint8)
    vis = accel.DeviceArray(ctx, (C, B), np.complex64)
    vis.set(q, vis_host)
    flags = accel.DeviceArray(ctx, (C, B), np.uint8)
    flags.set(q, flags_host)
    tuning = {"wgs": 64, "csplit": 0}

    ops = []  # (name, width, mode, operation)
    for mode in ("NONE", "FULL"):
        for width in WIDTHS:
            t = device.BackgroundMedianFilterDeviceTemplate(
                ctx, width, False, device.BackgroundFlags[mode], tuning=tuning)
            op = t.instantiate(q, C, B)
            op.bind(vis=vis)
            if mode == "FULL":
                op.bind(flags=flags)
            op.ensure_all_bound()
            ops.append(("background", width, mode, op))
    for width in SEQ_WIDTHS:
        t = device.FlaggerDeviceTemplate(
            device.BackgroundMedianFilterDeviceTemplate(ctx, width, tuning=tuning),
            device.NoiseEstMADTDeviceTemplate(ctx, 10240, tuning={"wgsx": 256}),
            device.ThresholdSumDeviceTemplate(ctx, tuning={"wgsx": 256, "vt": 0}),
            fused=False)
        op = t.instantiate(q, C, B, threshold_args={"n_sigma": 11.0})
        assert isinstance(op, device.FlaggerDevice)
        op.bind(vis=vis)
        op.ensure_all_bound()
        ops.append(("sequence", width, "NONE", op))

    for _, _, _, op in ops:  # warm-up: code objects loaded, clocks up
        for _ in range(5):
            op()
    q.finish()
    times = {i: [] for i in range(len(ops))}
    for _ in range(rounds):
        for i, (_, _, _, op) in enumerate(ops):
            a = q.enqueue_marker()
            for _ in range(CALLS):
                op()
            b = q.enqueue_marker()
            q.finish()
            times[i].append(1e3 * b.time_since(a) / CALLS)

    # the outputs of the last timed call, against the oracle
    oracle.set_threads(min(oracle.max_threads(), 16))
    checked = {}
    for i, (kind, width, mode, op) in enumerate(ops):
        t0 = time.time()
        dev = op.buffer("deviations").get(q)
        ok = True
        for sl in SLICES:
            v = np.ascontiguousarray(vis_host[:, sl])
            f = np.ascontiguousarray(flags_host[:, sl]) if mode == "FULL" else None
            dev32 = oracle.BackgroundMedianFilterHost(width)(v, f).astype(np.float32)
            ok &= np.array_equal(dev32, dev[:, sl])
            if kind == "sequence":
                noise32 = oracle.NoiseEstMADHost()(dev32).astype(np.float32)
                fl = oracle.ThresholdSumHost(11.0)(dev32, noise32)
                ok &= np.array_equal(noise32, op.buffer("noise").get(q)[sl])
                ok &= np.array_equal(fl, op.buffer("flags").get(q)[:, sl])
        checked[i] = (ok, time.time() - t0)

    print(f"# {ctx.device.name}: {C} channels x {B} baselines complex64, {rounds} rounds x "
          f"{CALLS} calls per configuration, alternating; median (min) ms per call")
    med = {}
    for i, (kind, width, mode, _) in enumerate(ops):
        ts = np.array(times[i])
        med[(kind, width, mode)] = float(np.median(ts))
        ok, secs = checked[i]
        ns = 1e6 * med[(kind, width, mode)] / (C * B)
        print(f"{kind:10s} width {width:3d} flags {mode:4s}  {np.median(ts):8.4f} ms "
              f"({ts.min():8.4f})  {ns:7.4f} ns/sample  oracle slices: "
              f"{'match' if ok else 'MISMATCH'} ({secs:.1f} s)")
    for mode in ("NONE", "FULL"):
        t31, t33 = med[("background", 31, mode)], med[("background", 33, mode)]
        t255 = med[("background", 255, mode)]
        print(f"flags {mode}: t(33)/t(31) = {t33 / t31:.2f} (bound 3), "
              f"t(255)/t(33) = {t255 / t33:.2f} (bound 10)")
    if not all(ok for ok, _ in checked.values()):
        sys.exit(1)


if __name__ == "__main__":
    main()
