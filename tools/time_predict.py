#!/usr/bin/env python3
"""Time the prediction of model visibilities (``rfi.ingest.PredictTemplate``) against a
streaming kernel, and count what it does.

Device time from events on one stream, data resident on the device, after a warm-up; every
figure is the median over ROUNDS rounds of CALLS calls, with the fastest and slowest round
beside it as the run-to-run spread. Shapes: 1024 x 32768 with 1, 4 and 16 sources (a band
around 1.4 GHz, delays of up to a microsecond). Two variants: the model alone (8 bytes written
per sample) and the division without a model output, with weights and flags (13 bytes read and
13 written per sample), out of place. The result of the warm-up call is compared with
``rfi.host.PredictHost`` on sampled rows, bit for bit (a NaN for a NaN).

Reported per variant: milliseconds, (sample, source) pairs per second, float64 operations per
second at FLOPS_PER_PAIR operations per pair (counted from csrc/predict.hip: PR_FLOPS_PER_PAIR)
and their share of FP64_PEAK, and bytes per second with their share of HBM_PEAK. Timed in
alternation with the operation, in the same rounds: the float32 transpose of the same shape,
which reads 4 and writes 4 bytes per sample, as the yardstick for streaming speed.

Every shape is measured in a process of its own, started under a time limit; the first one
that fails ends the run.

Usage: ``python tools/time_predict.py [--rounds N] [--calls N] [--json OUT] [--shape CxBxN ...]``.
"""

import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = ["1024x32768x1", "1024x32768x4", "1024x32768x16"]
SAMPLED_ROWS = 6
CHILD_SECONDS = 300
FLOPS_PER_PAIR = 36
FP64_PEAK = 78.6e12  # vector float64, operations per second: half the float32 vector rate
HBM_PEAK = 8.0e12  # bytes per second
#: name, (model, divide, weights, flags), bytes per sample
VARIANTS = [("model", (True, False, False, False), 8), ("divide", (False, True, True, True), 26)]


def measure(channels, baselines, n_sources, rounds, calls):
    """One shape, both variants, in this process."""
    import numpy as np

    from katsdpsigproc_amd import accel, transpose
    from katsdpsigproc_amd.rfi import host, ingest

    def time_rounds(queue, functions):
        times = [[] for _ in functions]
        for _ in range(rounds):
            for i, fn in enumerate(functions):
                start = queue.enqueue_marker()
                for _ in range(calls):
                    fn()
                stop = queue.enqueue_marker()
                times[i].append(stop.time_since(start) / calls * 1e3)
        return [{"median_ms": float(np.median(t)), "min_ms": min(t), "max_ms": max(t)}
                for t in times]  # fmt: skip

    def same(want, got, what):
        want, got = np.ascontiguousarray(want), np.ascontiguousarray(got)
        if want.dtype == np.uint8:
            assert np.array_equal(want, got), what
            return
        nan = np.isnan(want.view(np.float32))
        equal = want.view(np.uint32) == got.view(np.uint32)
        assert np.all(np.where(nan, np.isnan(got.view(np.float32)), equal)), what

    samples = channels * baselines
    context = accel.create_some_context(interactive=False)
    queue = context.create_command_queue()
    rs = np.random.RandomState(1)
    shape = (channels, baselines)
    case = {"freqs": np.linspace(1.2e9, 1.6e9, channels),
            "delays": rs.uniform(-1e-6, 1e-6, (n_sources, baselines)),
            "flux": np.exp2(rs.uniform(-2, 2, (channels, n_sources))).astype(np.float32)}  # fmt: skip
    vis = np.empty(shape, np.complex64)
    vis.real[...] = rs.random_sample(shape).astype(np.float32) - 0.5
    vis.imag[...] = vis.real[::-1]
    data = {"vis": vis, "weights": np.exp2(6 * vis.real).astype(np.float32),
            "flags": ((vis.real > 0.4) * 3).astype(np.uint8)}  # fmt: skip
    rows = np.unique(rs.randint(0, channels, SAMPLED_ROWS))
    want = host.PredictHost()(case["freqs"][rows], case["delays"], case["flux"][rows],
                              *(data[name][rows] for name in ("vis", "weights", "flags")))  # fmt: skip
    want = dict(zip(("model", "out_vis", "out_weights", "out_flags"), want))
    yardstick = transpose.TransposeTemplate(context, np.float32, "float").instantiate(queue, shape)
    yardstick.ensure_all_bound()
    yardstick.buffer("src").set(queue, data["weights"])

    runs = []
    for name, variant, per_sample in VARIANTS:
        op = ingest.PredictTemplate(context, *variant).instantiate(
            queue, channels, baselines, n_sources)  # fmt: skip
        op.ensure_all_bound()
        for slot in op.slots:
            if slot in case or slot in data:
                op.buffer(slot).set(queue, case.get(slot, data.get(slot)))
        op()
        queue.finish()
        for slot in op.slots:
            if slot in want:
                same(want[slot], op.buffer(slot).get(queue)[rows], slot)
        for _ in range(2):
            yardstick()
            op()
        queue.finish()
        timed = time_rounds(queue, [op, yardstick])
        seconds = timed[0]["median_ms"] * 1e-3
        pairs = samples * n_sources
        run = {"variant": name, "bytes_per_sample": per_sample, "op": timed[0],
               "transpose": timed[1], "pairs_per_s": pairs / seconds,
               "flops_per_pair": FLOPS_PER_PAIR, "flops_per_s": pairs * FLOPS_PER_PAIR / seconds,
               "bytes_per_s": samples * per_sample / seconds}  # fmt: skip
        run["fp64_peak_fraction"] = run["flops_per_s"] / FP64_PEAK
        run["hbm_peak_fraction"] = run["bytes_per_s"] / HBM_PEAK
        run["transpose"]["bytes_per_s"] = samples * 8 / (timed[1]["median_ms"] * 1e-3)
        runs.append(run)
        del op
    return {"device": context.device.name, "channels": channels, "baselines": baselines,
            "n_sources": n_sources, "rounds": rounds, "calls": calls, "verified": True,
            "variants": runs}  # fmt: skip


def text(entry):
    return f"{entry['median_ms']:.3f} ms ({entry['min_ms']:.3f}..{entry['max_ms']:.3f})"


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--shape", action="append", help="CHANNELSxBASELINESxSOURCES (repeatable)")
    parser.add_argument("--rounds", type=int, default=5)
    parser.add_argument("--calls", type=int, default=10)
    parser.add_argument("--json")
    parser.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    args = parser.parse_args()
    shapes = args.shape or SHAPES
    if args.child:
        channels, baselines, n_sources = (int(n) for n in shapes[0].split("x"))
        print(json.dumps(measure(channels, baselines, n_sources, args.rounds, args.calls)))
        return
    results = []
    for shape in shapes:
        command = ["timeout", "-k", "10", str(CHILD_SECONDS), sys.executable,
                   os.path.abspath(__file__), "--child", "--shape", shape,
                   "--rounds", str(args.rounds), "--calls", str(args.calls)]  # fmt: skip
        done = subprocess.run(command, stdout=subprocess.PIPE, text=True)
        if done.returncode != 0:
            sys.exit(f"{shape}: exit status {done.returncode}; nothing more is started")
        result = json.loads(done.stdout.strip().splitlines()[-1])
        print(f"{shape}:")
        for run in result["variants"]:
            print(f"  {run['variant']:6s}: op {text(run['op'])}, "
                  f"{run['pairs_per_s'] / 1e9:.1f} G pairs/s, "
                  f"{run['flops_per_s'] / 1e12:.2f} T float64 op/s "
                  f"({100 * run['fp64_peak_fraction']:.1f} % of {FP64_PEAK / 1e12:.1f}), "
                  f"{run['bytes_per_s'] / 1e12:.2f} TB/s "
                  f"({100 * run['hbm_peak_fraction']:.1f} % of {HBM_PEAK / 1e12:.0f}); transpose "
                  f"{text(run['transpose'])}, {run['transpose']['bytes_per_s'] / 1e12:.2f} TB/s",
                  flush=True)  # fmt: skip
        results.append(result)
    if args.json:
        with open(args.json, "w") as f:
            json.dump({"runs": results}, f, indent=1)


if __name__ == "__main__":
    main()
