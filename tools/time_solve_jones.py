#!/usr/bin/env python3
"""Time the Jones solver (``rfi.ingest.SolveJonesTemplate``) against the scalar solver
(``rfi.ingest.SolveGainsTemplate``) on the same arrays.

Device time from events on one stream, data resident on the device, after a warm-up; every
figure is the median over ROUNDS rounds of CALLS calls, with the fastest and slowest round
beside it as the run-to-run spread. Shapes: 4096 channels x 2016 baselines with 64 inputs (32
dual-feed antennas) and 4096 x 8256 with 128 inputs (every pair of inputs; the second with the
autocorrelations, which take no part).
The data are ``J_a J_b^H`` of matrices with diagonals of magnitude 0.5 .. 2 and leakage of up to
0.1 plus 1 % noise, with weights and flags (2 % flagged); both solvers start from the identity
with the default ``tol=1e-5`` and ``max_iterations=30``. The result of the warm-up call is
compared with ``rfi.host.SolveJonesHost`` on sampled channels, bit for bit.

Timed in alternation, in the same rounds: the Jones solver, the Jones solver with
``max_iterations=1`` (the load phase and one iteration, what the launch costs before it
iterates), the scalar solver on the same ``vis``, ``weights``, ``flags`` and ``pairs``, and the
scalar solver with ``max_iterations=1``. The iteration counts of both are reported: the two do
not run the same number, so the time per iteration is the comparison.

Every shape is measured in a process of its own, started under a time limit; the first one
that fails ends the run.

Usage: ``python tools/time_solve_jones.py [--rounds N] [--calls N] [--json OUT]
[--shape CxBxN ...]``.
"""

import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = ["4096x2016x64", "4096x8256x128"]
SAMPLED_CHANNELS = 4
CHILD_SECONDS = 400


def measure(channels, baselines, n_inputs, rounds, calls):
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
    autos = baselines >= n_inputs * (n_inputs + 1) // 2
    listed = [(a, b) for a in range(n_inputs) for b in range(a if autos else a + 1, n_inputs)]
    assert len(listed) <= baselines, "fewer baselines than pairs of inputs"
    inputs = np.zeros((baselines, 2), np.int32)  # (the rest: autocorrelations of input 0)
    inputs[: len(listed)] = listed
    pairs = host.SolveJonesHost.pair_table(inputs, n_inputs)
    shape = (channels, n_inputs)
    diagonal = rs.uniform(0.5, 2, shape) * np.exp(2j * np.pi * rs.uniform(0, 1, shape))
    leak = rs.uniform(0, 0.1, shape) * np.exp(2j * np.pi * rs.uniform(0, 1, shape))
    truth = np.empty(shape + (2,), np.complex128)
    feed = np.arange(n_inputs) % 2
    truth[:, np.arange(n_inputs), feed] = diagonal
    truth[:, np.arange(n_inputs), 1 - feed] = diagonal * leak
    vis = np.empty((channels, baselines), np.complex64)
    weights = np.empty((channels, baselines), np.float32)
    flags = np.empty((channels, baselines), np.uint8)
    for r0 in range(0, channels, 256):
        rows = slice(r0, r0 + 256)
        z = truth[rows]
        part = (z[:, inputs[:, 0]] * np.conj(z[:, inputs[:, 1]])).sum(axis=2)
        part += 0.01 * (rs.standard_normal(part.shape) + 1j * rs.standard_normal(part.shape))
        vis[rows] = part
        weights[rows] = np.exp2(rs.uniform(-2, 2, part.shape))
        flags[rows] = (rs.random_sample(part.shape) < 0.02) * np.uint8(4)

    context = accel.create_some_context(interactive=False)
    queue = context.create_command_queue()
    args = (queue, channels, baselines, n_inputs)
    op = ingest.SolveJonesTemplate(context).instantiate(*args)
    op.ensure_all_bound()
    once = ingest.SolveJonesTemplate(context, max_iterations=1).instantiate(*args)
    once.bind(**{name: op.buffer(name) for name in op.slots})
    shared = {name: op.buffer(name) for name in ("vis", "weights", "flags", "pairs")}
    scalar = ingest.SolveGainsTemplate(context).instantiate(*args)
    scalar.bind(**shared)
    scalar.ensure_all_bound()
    scalar_once = ingest.SolveGainsTemplate(context, max_iterations=1).instantiate(*args)
    scalar_once.bind(**{name: scalar.buffer(name) for name in scalar.slots})
    for name, value in (("vis", vis), ("weights", weights), ("flags", flags), ("pairs", pairs)):
        op.buffer(name).set(queue, value)

    op()
    scalar()
    queue.finish()
    jones = op.buffer("jones").get(queue)
    iterations = op.buffer("iterations").get(queue)
    status = op.buffer("status").get(queue)
    scalar_iterations = scalar.buffer("iterations").get(queue)
    sampled = np.unique(rs.randint(0, channels, SAMPLED_CHANNELS))
    want = host.SolveJonesHost()(vis[sampled], pairs, weights[sampled], flags[sampled])
    nan = np.isnan(want[0].view(np.float32))
    got = np.ascontiguousarray(jones[sampled])
    assert np.all(np.where(nan, np.isnan(got.view(np.float32)),
                           want[0].view(np.uint32) == got.view(np.uint32)))  # fmt: skip
    assert np.array_equal(want[1], iterations[sampled])
    assert np.array_equal(want[2], status[sampled])
    # J_a J_b^H against the truth's, between different antennas, on the sampled channels
    j = got.astype(np.complex128).reshape(len(sampled), n_inputs // 2, 2, 2)
    t = truth[sampled].reshape(len(sampled), n_inputs // 2, 2, 2)
    product = np.einsum("caik,cbjk->cabij", j, np.conj(j))
    model = np.einsum("caik,cbjk->cabij", t, np.conj(t))
    off = ~np.eye(n_inputs // 2, dtype=bool)
    error = float(np.abs(product - model)[:, off].max())

    functions = [op, once, scalar, scalar_once]
    for _ in range(2):
        for fn in functions:
            fn()
    queue.finish()
    timed = time_rounds(queue, functions)
    result = {"device": context.device.name, "channels": channels, "baselines": baselines,
              "n_inputs": n_inputs, "rounds": rounds, "calls": calls, "verified": True,
              "iterations_min": int(iterations.min()), "iterations_max": int(iterations.max()),
              "iterations_mean": float(iterations.mean()),
              "not_converged": int(np.count_nonzero(status & 1)),
              "scalar_iterations_mean": float(scalar_iterations.mean()),
              "largest_error_of_the_products": error,
              "op": timed[0], "op_one_iteration": timed[1], "scalar": timed[2],
              "scalar_one_iteration": timed[3]}  # fmt: skip
    result["ms_per_iteration"] = (
        (timed[0]["median_ms"] - timed[1]["median_ms"]) / (result["iterations_mean"] - 1))
    result["scalar_ms_per_iteration"] = (
        (timed[2]["median_ms"] - timed[3]["median_ms"]) / (result["scalar_iterations_mean"] - 1))
    result["op_over_scalar"] = timed[0]["median_ms"] / timed[2]["median_ms"]
    return result


def text(entry):
    return f"{entry['median_ms']:.3f} ms ({entry['min_ms']:.3f}..{entry['max_ms']:.3f})"


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--shape", action="append", help="CHANNELSxBASELINESxINPUTS (repeatable)")
    parser.add_argument("--rounds", type=int, default=5)
    parser.add_argument("--calls", type=int, default=10)
    parser.add_argument("--json")
    parser.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    args = parser.parse_args()
    shapes = args.shape or SHAPES
    if args.child:
        channels, baselines, n_inputs = (int(n) for n in shapes[0].split("x"))
        print(json.dumps(measure(channels, baselines, n_inputs, args.rounds, args.calls)))
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
        print(f"{shape}: {r['iterations_min']}..{r['iterations_max']} iterations (mean "
              f"{r['iterations_mean']:.1f}; scalar solver mean {r['scalar_iterations_mean']:.1f}), "
              f"{r['not_converged']} channels not converged, largest error of J J^H "
              f"{r['largest_error_of_the_products']:.2e}\n"
              f"  jones {text(r['op'])}; one iteration {text(r['op_one_iteration'])}; "
              f"{r['ms_per_iteration']:.4f} ms per further iteration\n"
              f"  scalar {text(r['scalar'])}; one iteration {text(r['scalar_one_iteration'])}; "
              f"{r['scalar_ms_per_iteration']:.4f} ms per further iteration; jones / scalar = "
              f"{r['op_over_scalar']:.2f}", flush=True)  # fmt: skip
        results.append(r)
    if args.json:
        with open(args.json, "w") as f:
            json.dump({"runs": results}, f, indent=1)


if __name__ == "__main__":
    main()
