#!/usr/bin/env python3
"""Diagnostic: SumThreshold on channel-major deviations (``ThresholdSumDeviceTemplate(
transposed=False)``, one kernel) against what a channel-major pipeline did before: transpose the
deviations, the baseline-major kernel, transpose the flags back. 4096 x 8192 and 32768 x 4096
(channels x baselines), 4 and 8 windows, on unit noise and on the RFI-laden block (1/16 of
the samples raised by 50-70 sigma), 11 sigma. Then the kernel-per-stage flagger at width 63
with each threshold layout. Alternating rounds; median (min) ms per call. Every pair of
paths is checked to give the same flags."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from katsdpsigproc_amd import _lib  # noqa: E402

if os.environ.get("KSP_LIB"):
    _lib.load(os.path.abspath(os.environ["KSP_LIB"]))
from katsdpsigproc_amd import accel, transpose  # noqa: E402
from katsdpsigproc_amd.rfi import device  # noqa: E402

ROUNDS, CALLS = 7, 5

ctx = accel.create_some_context(False)
q = ctx.create_command_queue()


def timed(run):
    for _ in range(20):  # sustained clocks
        run()
    q.finish()
    return run


def measure(runs):
    """{label: [ms per call, one per round]}, the labels alternating within each round."""
    out = {label: [] for label in runs}
    for _ in range(ROUNDS):
        for label, run in runs.items():
            a = q.enqueue_marker()
            for _ in range(CALLS):
                run()
            b = q.enqueue_marker()
            q.finish()
            out[label].append(1e3 * b.time_since(a) / CALLS)
    return out


def deviations(C, B, rfi):
    rs = np.random.RandomState(1)
    dev = np.empty((C, B), np.float32)
    for r0 in range(0, C, 1024):
        dev[r0 : r0 + 1024] = rs.standard_normal((min(1024, C - r0), B))
        if rfi:
            part = dev[r0 : r0 + 1024]
            hit = rs.random_sample(part.shape) < 1 / 16
            part[hit] += (rs.random_sample(int(hit.sum())) * 20 + 50).astype(np.float32)
    return dev


def threshold_pair(C, B, n_windows, dev):
    noise = np.ones(B, np.float32)
    cm = device.ThresholdSumDeviceTemplate(ctx, n_windows, transposed=False).instantiate(q, C, B, 11.0)
    cm.ensure_all_bound()
    cm.buffer("deviations").set(q, dev)
    cm.buffer("noise").set(q, noise)
    bm = device.ThresholdSumDeviceTemplate(ctx, n_windows, tuning={"vt": 0}).instantiate(q, C, B, 11.0)
    t_dev = transpose.TransposeTemplate(ctx, np.float32, "float").instantiate(q, (C, B))
    t_flags = transpose.TransposeTemplate(ctx, np.uint8, "unsigned char").instantiate(q, (B, C))
    t_dev.bind(src=cm.buffer("deviations"))
    t_dev.ensure_all_bound()
    bm.bind(deviations=t_dev.buffer("dest"), noise=cm.buffer("noise"))
    bm.ensure_all_bound()
    t_flags.bind(src=bm.buffer("flags"))
    t_flags.ensure_all_bound()

    def run_bm():
        t_dev()
        bm()
        t_flags()

    runs = {"channel-major kernel": timed(cm), "transpose + kernel + transpose": timed(run_bm)}
    got, ref = cm.buffer("flags").get(q), t_flags.buffer("dest").get(q)
    same = np.array_equal(got, ref)
    return runs, same, np.count_nonzero(got) / got.size


def flagger_runs(C, B):
    from tests import inputs

    vis = inputs.add_rfi(inputs.generate_data(C, B, seed=1))
    runs, flags = {}, {}
    for label, ne, transposed in (
        ("sequence MADT + SumThreshold baseline-major", "MADT", True),
        ("sequence MADT + SumThreshold channel-major", "MADT", False),
        ("sequence MAD  + SumThreshold channel-major", "MAD", False),
    ):
        if ne == "MADT":
            noise_est = device.NoiseEstMADTDeviceTemplate(ctx, C, tuning={"wgsx": 256})
        else:
            noise_est = device.NoiseEstMADDeviceTemplate(ctx, tuning={"method": 0})
        tmpl = device.FlaggerDeviceTemplate(
            device.BackgroundMedianFilterDeviceTemplate(ctx, 63, tuning={"wgs": 64, "csplit": 0}),
            noise_est,
            device.ThresholdSumDeviceTemplate(ctx, 4, tuning={"vt": 0}, transposed=transposed),
            fused=False,
        )
        fn = tmpl.instantiate(q, C, B, threshold_args={"n_sigma": 11.0})
        fn.ensure_all_bound()
        fn.buffer("vis").set(q, vis)
        runs[label] = timed(fn)
        flags[label] = fn.buffer("flags")
    values = [f.get(q) for f in flags.values()]
    same = all(np.array_equal(values[0], v) for v in values[1:])
    return runs, same


def report(prefix, results, extra=""):
    for label, ms in results.items():
        print(f"{prefix} {label:44s} {np.median(ms):8.4f} ms ({min(ms):8.4f}){extra}", flush=True)


print(f"# {ctx.device.name}: {ROUNDS} rounds x {CALLS} calls per path, alternating; "
      "median (min) ms per call")
for C, B in ((4096, 8192), (32768, 4096)):
    for rfi in (False, True):
        dev = deviations(C, B, rfi)
        for n_windows in (4, 8):
            runs, same, frac = threshold_pair(C, B, n_windows, dev)
            res = measure(runs)
            tag = f"{C:5d} x {B:4d} {'rfi  ' if rfi else 'noise'} {n_windows} windows:"
            report(tag, res, f"  flagged {frac:.4f}  flags equal: {same}")
            ratio = np.median(res["channel-major kernel"]) / np.median(
                res["transpose + kernel + transpose"])
            print(f"{tag} ratio channel-major / transposing = {ratio:.2f}", flush=True)
            del runs
for C, B in ((4096, 8192),):
    runs, same = flagger_runs(C, B)
    report(f"{C:5d} x {B:4d} width 63 rfi:", measure(runs), f"  flags equal: {same}")
