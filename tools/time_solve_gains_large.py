#!/usr/bin/env python3
"""Time the gain solver for large arrays (``rfi.ingest.SolveGainsLargeTemplate``) against the
bytes its iterations must move and against the NumPy host class.

Device time from events on one stream, data resident on the device, after a warm-up; every
figure is the median over ROUNDS rounds of CALLS calls, with the fastest and slowest round
beside it as the run-to-run spread. Shapes: 4096 channels with 160, 394 and 512 inputs and
every pair of inputs as a baseline (12720, 77421 and 130816 baselines).
The data are ``g_a conj(g_b)`` of gains of magnitude 0.5 .. 2 plus 1 % noise, with weights and
flags (2 % flagged); DISTINCT_CHANNELS channels are made and repeated to fill the array (the
host has to make them; the device reads every channel from its own addresses). The solver
starts from unit gains with the default ``tol=1e-5`` and ``max_iterations=30``. The result of
the warm-up call is compared with ``rfi.host.SolveGainsLargeHost`` on sampled channels, bit for
bit.

Timed in alternation with the operation, in the same rounds: the operation with
``max_iterations=1``, which fills every channel's matrix and runs one iteration.

An iteration reads a channel's matrix once, three float32 planes of n_inputs x n_inputs
elements, so the iterations of a call must move ``sum(iterations) * 12 * n_inputs^2`` bytes
(the fill writes the matrix once more and gathers 13 bytes per sample twice; neither is
counted); the tool reports that over the operation's time.

The host class is timed on the CPU on HOST_CHANNELS channels and scaled to the whole array.
Every shape is measured in a process of its own, started under a time limit; the first one
that fails ends the run.

Usage: ``python tools/time_solve_gains_large.py [--rounds N] [--calls N] [--json OUT]
[--shape CxN ...]``.
"""

import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = ["4096x160", "4096x394", "4096x512"]
SAMPLED_CHANNELS = 4
HOST_CHANNELS = 8
DISTINCT_CHANNELS = 256
CHILD_SECONDS = 400


def measure(channels, n_inputs, rounds, calls):
    """One shape in this process."""
    import numpy as np

    from katsdpsigproc_amd import accel
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

    rs = np.random.RandomState(1)
    inputs = np.ascontiguousarray(np.array(np.triu_indices(n_inputs, 1)).T, np.int32)
    baselines = len(inputs)
    pairs = host.SolveGainsLargeHost.pair_table(inputs, n_inputs)
    distinct = min(DISTINCT_CHANNELS, channels)
    shape = (distinct, n_inputs)
    truth = (rs.uniform(0.5, 2, shape) * np.exp(2j * np.pi * rs.uniform(0, 1, shape)))
    vis = np.empty((channels, baselines), np.complex64)
    weights = np.empty((channels, baselines), np.float32)
    flags = np.empty((channels, baselines), np.uint8)
    for r0 in range(0, distinct, 64):
        rows = slice(r0, min(r0 + 64, distinct))
        g = truth[rows]
        part = g[:, inputs[:, 0]] * np.conj(g[:, inputs[:, 1]])
        part += 0.01 * (rs.standard_normal(part.shape) + 1j * rs.standard_normal(part.shape))
        vis[rows] = part
        weights[rows] = np.exp2(rs.uniform(-2, 2, part.shape))
        flags[rows] = (rs.random_sample(part.shape) < 0.02) * np.uint8(4)
    for r0 in range(distinct, channels, distinct):
        rows = slice(r0, min(r0 + distinct, channels))
        count = rows.stop - rows.start
        vis[rows], weights[rows], flags[rows] = vis[:count], weights[:count], flags[:count]
    truth = np.resize(truth, (channels, n_inputs))

    context = accel.create_some_context(interactive=False)
    queue = context.create_command_queue()
    op = ingest.SolveGainsLargeTemplate(context).instantiate(queue, channels, baselines, n_inputs)
    op.ensure_all_bound()
    once = ingest.SolveGainsLargeTemplate(context, max_iterations=1).instantiate(
        queue, channels, baselines, n_inputs)  # fmt: skip
    once.bind(**{name: op.buffer(name) for name in op.slots})
    for name, value in (("vis", vis), ("weights", weights), ("flags", flags), ("pairs", pairs)):
        op.buffer(name).set(queue, value)

    op()
    queue.finish()
    gains = op.buffer("gains").get(queue)
    iterations = op.buffer("iterations").get(queue)
    status = op.buffer("status").get(queue)
    sampled = np.unique(rs.randint(0, channels, SAMPLED_CHANNELS))
    want = host.SolveGainsLargeHost()(vis[sampled], pairs, weights[sampled], flags[sampled])
    nan = np.isnan(want[0].view(np.float32))
    got = np.ascontiguousarray(gains[sampled])
    assert np.all(np.where(nan, np.isnan(got.view(np.float32)),
                           want[0].view(np.uint32) == got.view(np.uint32)))  # fmt: skip
    assert np.array_equal(want[1], iterations[sampled])
    assert np.array_equal(want[2], status[sampled])
    turned = truth * np.conj(truth[:, :1]) / np.abs(truth[:, :1])
    error = float(np.abs(gains - turned).max())

    for _ in range(2):
        once()
        op()
    queue.finish()
    timed = time_rounds(queue, [op, once])

    few = slice(0, min(HOST_CHANNELS, channels))
    start = time.perf_counter()
    host.SolveGainsLargeHost()(vis[few], pairs, weights[few], flags[few])
    host_s = (time.perf_counter() - start) * channels / (few.stop - few.start)

    matrix_bytes = 12 * n_inputs * n_inputs
    moved = int(iterations.sum(dtype=np.int64)) * matrix_bytes
    result = {"device": context.device.name, "channels": channels, "baselines": baselines,
              "n_inputs": n_inputs, "rounds": rounds, "calls": calls, "verified": True,
              "distinct_channels": distinct,
              "iterations_min": int(iterations.min()), "iterations_max": int(iterations.max()),
              "iterations_mean": float(iterations.mean()),
              "not_converged": int(np.count_nonzero(status & 1)),
              "largest_error_against_the_true_gains": error,
              "work_bytes": ingest.SolveGainsLarge.work_bytes(channels, n_inputs),
              "matrix_bytes": matrix_bytes, "iteration_bytes": moved,
              "op": timed[0], "op_one_iteration": timed[1], "host_ms_scaled": host_s * 1e3,
              "host_channels": few.stop - few.start}  # fmt: skip
    result["op"]["iteration_bytes_per_s"] = moved / (timed[0]["median_ms"] * 1e-3)
    result["op_one_iteration"]["iteration_bytes_per_s"] = (
        channels * matrix_bytes / (timed[1]["median_ms"] * 1e-3))
    result["host_over_op"] = host_s * 1e3 / timed[0]["median_ms"]
    return result


def text(entry):
    return f"{entry['median_ms']:.3f} ms ({entry['min_ms']:.3f}..{entry['max_ms']:.3f})"


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--shape", action="append", help="CHANNELSxINPUTS (repeatable)")
    parser.add_argument("--rounds", type=int, default=5)
    parser.add_argument("--calls", type=int, default=10)
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
        r = json.loads(done.stdout.strip().splitlines()[-1])
        print(f"{shape}: {r['baselines']} baselines, {r['iterations_min']}..{r['iterations_max']} "
              f"iterations (mean {r['iterations_mean']:.1f}), {r['not_converged']} channels not "
              f"converged, largest error {r['largest_error_against_the_true_gains']:.2e}, work "
              f"area {r['work_bytes'] / 2**20:.0f} MiB\n"
              f"  op {text(r['op'])}, {r['op']['iteration_bytes_per_s'] / 1e12:.2f} TB/s of "
              f"matrix reads; one iteration {text(r['op_one_iteration'])}, "
              f"{r['op_one_iteration']['iteration_bytes_per_s'] / 1e12:.2f} TB/s; host class "
              f"{r['host_ms_scaled']:.0f} ms (scaled from {r['host_channels']} channels), "
              f"{r['host_over_op']:.0f} x", flush=True)  # fmt: skip
        results.append(r)
    if args.json:
        with open(args.json, "w") as f:
            json.dump({"runs": results}, f, indent=1)


if __name__ == "__main__":
    main()
