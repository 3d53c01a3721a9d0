#!/usr/bin/env python3
"""Time the filling of solved Jones matrices (``rfi.ingest.InterpolateJonesTemplate``) against
the round trip it removes.

Device time from events on one stream, data resident on the device, after a warm-up; every
figure is the median over ROUNDS rounds of CALLS calls, with the fastest and slowest round
beside it as the run-to-run spread. Shape: 4096 channels x 128 inputs (64 antennas), a smooth
bandpass per element with leakage of up to 0.1 and a delay per feed, with noise, about a sixth
of the channels missing in runs of up to 8 (the whole matrices NaN, and marked in ``status``),
with ``status``, ``model``, ``normalise`` and ``corrections``, ``max_gap`` 8, ``smooth`` 1 and 9;
and ``smooth`` 1 without ``model`` and ``normalise`` (the fill and the inverse alone). The
result of the warm-up call is compared with ``rfi.host.InterpolateJonesHost``, every output bit
for bit (a NaN for a NaN). ``rfi.ingest.InterpolateGains`` on the same channels x inputs is
timed beside it: a quarter of the elements.

Timed in alternation with the operation, in the same rounds: the round trip the operation
removes, ``jones``, ``status`` and ``model`` copied to the host and the corrections copied back
(wall-clock time of the four blocking copies, pageable host memory, without the host's
arithmetic).

Every shape is measured in a process of its own, started under a time limit; the first one
that fails ends the run.

Usage: ``python tools/time_interpolate_jones.py [--rounds N] [--calls N] [--json OUT]
[--shape CHANNELSxINPUTS ...]``.
"""

import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = ["4096x128"]
MAX_GAP = 8
#: (smooth, model and normalise)
VARIANTS = [(1, True), (9, True), (1, False)]
CHILD_SECONDS = 300


def measure(channels, n_inputs, rounds, calls):
    """One shape, every variant, in this process."""
    import numpy as np

    from katsdpsigproc_amd import accel
    from katsdpsigproc_amd.rfi import host, ingest

    def summary(t):
        return {"median_ms": float(np.median(t)), "min_ms": min(t), "max_ms": max(t)}

    def same(want, got, what):
        want, got = np.ascontiguousarray(want), np.ascontiguousarray(got)
        if want.dtype.kind in "iu":
            assert np.array_equal(want, got), what
            return
        nan = np.isnan(want.view(np.float32))
        equal = want.view(np.uint32) == got.view(np.uint32)
        assert np.all(np.where(nan, np.isnan(got.view(np.float32)), equal)), what

    context = accel.create_some_context(interactive=False)
    queue = context.create_command_queue()
    rs = np.random.RandomState(1)
    c = np.arange(channels)[:, np.newaxis, np.newaxis]
    shape = (channels, n_inputs, 2)
    rotation = np.exp(2j * np.pi * (c * rs.uniform(-0.3, 0.3, (n_inputs, 1))
                                    + rs.random_sample((n_inputs, 1))))  # fmt: skip
    theta = 2 * np.pi * c / rs.uniform(500, 2000, (n_inputs, 2))
    leak = rs.uniform(0.01, 0.1, (n_inputs, 2)) * np.exp(2j * np.pi * rs.random_sample((n_inputs, 2)))
    leak[np.arange(n_inputs), np.arange(n_inputs) % 2] = 1
    jones = (1 + 0.2 * np.cos(theta)) * np.exp(0.3j * np.sin(theta)) * leak * rotation
    jones += 0.02 * (rs.standard_normal(shape) + 1j * rs.standard_normal(shape))
    jones = jones.astype(np.complex64)
    model = np.ascontiguousarray(rotation[:, :, 0].astype(np.complex64))
    status = np.zeros(channels, np.uint8)
    at = 5
    while at < channels - MAX_GAP:
        length = rs.randint(1, MAX_GAP + 1)
        status[at : at + length] = 2
        at += length + rs.randint(1, 6 * MAX_GAP)
    jones[status != 0] = complex(np.nan, np.nan)
    names = ("out", "kept", "filled", "fill_status", "mean_amplitude")

    runs = []
    for smooth, full in VARIANTS:
        op = ingest.InterpolateJonesTemplate(context, MAX_GAP, smooth, full, True, 0xFF, full,
                                             False, True).instantiate(queue, channels, n_inputs)  # fmt: skip
        scalar = ingest.InterpolateGainsTemplate(context, MAX_GAP, smooth, full, True, 0xFF, full,
                                                 False, True).instantiate(queue, channels, n_inputs)  # fmt: skip
        op.ensure_all_bound()
        scalar.ensure_all_bound()
        op.buffer("jones").set(queue, jones)
        scalar.buffer("gains").set(queue, host.JonesDiagonalHost()(jones))
        for fn in (op, scalar):
            fn.buffer("status").set(queue, status)
            if full:
                fn.buffer("model").set(queue, model)
        op()
        queue.finish()
        want = host.InterpolateJonesHost(MAX_GAP, smooth, full, 0xFF, True)(
            jones, status, model if full else None)  # fmt: skip
        for name, w in zip(names, want):
            if name in op.slots:
                same(w, op.buffer(name).get(queue), name)
        for _ in range(2):
            op()
            scalar()
        queue.finish()
        corrections = accel.DeviceArray(context, shape, np.complex64)
        times = {"op": [], "interpolate_gains": [], "round_trip": []}
        for _ in range(rounds):
            for name, fn in (("op", op), ("interpolate_gains", scalar)):
                start = queue.enqueue_marker()
                for _ in range(calls):
                    fn()
                stop = queue.enqueue_marker()
                times[name].append(stop.time_since(start) / calls * 1e3)
            queue.finish()
            begin = time.perf_counter()
            for _ in range(calls):
                op.buffer("jones").get(queue)
                op.buffer("status").get(queue)
                if full:
                    op.buffer("model").get(queue)
                corrections.set(queue, want[0])
            queue.finish()
            times["round_trip"].append((time.perf_counter() - begin) / calls * 1e3)
        run = {"smooth": smooth, "model": full, "normalise": full,
               "missing": int(np.count_nonzero(status)), "filled": int(want[2].sum()),
               "gaps_left": int(np.count_nonzero(want[3]))}  # fmt: skip
        run.update({name: summary(t) for name, t in times.items()})
        runs.append(run)
        del op, scalar
    return {"device": context.device.name, "channels": channels, "n_inputs": n_inputs,
            "max_gap": MAX_GAP, "rounds": rounds, "calls": calls, "verified": True,
            "runs": runs}  # fmt: skip


def text(entry):
    return f"{entry['median_ms']:.4f} ms ({entry['min_ms']:.4f}..{entry['max_ms']:.4f})"


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--shape", action="append", help="CHANNELSxINPUTS (repeatable)")
    parser.add_argument("--rounds", type=int, default=7)
    parser.add_argument("--calls", type=int, default=20)
    parser.add_argument("--json")
    parser.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    args = parser.parse_args()
    shapes = args.shape or SHAPES
    if args.child:
        channels, n_inputs = (int(n) for n in shapes[0].split("x"))
        print(json.dumps(measure(channels, n_inputs, args.rounds, args.calls)))
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
        for run in result["runs"]:
            variant = f"smooth {run['smooth']}" + (
                ", model, normalise" if run["model"] else ", the fill and the inverse alone")  # fmt: skip
            print(f"  {variant}: op {text(run['op'])}; interpolate_gains on the same inputs "
                  f"{text(run['interpolate_gains'])}; jones, status{', model' if run['model'] else ''}"
                  f" to the host and corrections back {text(run['round_trip'])}; "
                  f"{run['filled']} matrices filled, {run['gaps_left']} antennas with a gap left",
                  flush=True)  # fmt: skip
        results.append(result)
    if args.json:
        with open(args.json, "w") as f:
            json.dump({"runs": results}, f, indent=1)


if __name__ == "__main__":
    main()
