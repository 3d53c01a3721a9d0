#!/usr/bin/env python3
"""Time the application of Jones matrices (``rfi.ingest.ApplyJonesTemplate``) against the
application of gains on the same arrays, and against what a caller could do without it.

Device time from events on one stream, data resident on the device, after a warm-up; every
figure is the median over ROUNDS rounds of CALLS calls, with the fastest and slowest round
beside it as the run-to-run spread. Shapes: 4096 channels x 32 dual-feed antennas (2080
baselines, 528 quads) and x 64 antennas (8256 baselines, 2080 quads), all autocorrelations and
of a dish's cross hands (2a, 2a+1) alone, with the baselines in polarisation blocks
(``blocks``), with the four products of a pair adjacent (``adjacent``) and, as the bad case, in
a random order and direction (``random``). The matrices have diagonals around 1, leakage up to
0.1 and 1 % NaN. Weights and flags, out of place and in place. The result of the warm-up call
is compared with ``rfi.host.ApplyJonesHost`` on sampled rows, bit for bit (a NaN for a NaN).

Timed in alternation with the operation, in the same rounds:

* ``ApplyGains`` on the same sample arrays with the same ``inputs`` and one gain per input:
  the same 26 bytes per sample;
* the torch composite a caller can write today on tensors that wrap the operation's own
  buffers, for the visibilities alone: four gathers (one per product, conjugated where the
  table says so), two batched 2x2 matrix products and a scatter per product (not bit for bit
  the definition, no weights, no flags, no test for NaN).

Every case is measured in a process of its own, started under a time limit; the first one
that fails ends the run.

Usage: ``python tools/time_apply_jones.py [--rounds N] [--calls N] [--json OUT]
[--case CHANNELSxANTENNASxORDER ...]``.
"""

import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = ["4096x32xblocks", "4096x32xadjacent", "4096x64xblocks", "4096x64xadjacent",
         "4096x64xrandom"]  # fmt: skip
SAMPLED_ROWS = 6
CHILD_SECONDS = 300
FLAG_VALUE = 128
BYTES_PER_SAMPLE = 26


def layout(n_ant, order):
    """int32 (baselines, 2): every product of every pair a < b, and of a dish (2a, 2a),
    (2a+1, 2a+1) and (2a, 2a+1)."""
    import numpy as np

    pairs = [(a, b) for a in range(n_ant) for b in range(a, n_ant)]
    pols = [(0, 0), (1, 1), (0, 1), (1, 0)] if order == "blocks" else [(0, 0), (0, 1), (1, 0), (1, 1)]

    def listed(a, b, m, n):
        return a != b or (m, n) != (1, 0)

    if order == "blocks":
        inputs = [(2 * a + m, 2 * b + n) for m, n in pols for a, b in pairs if listed(a, b, m, n)]
    else:
        inputs = [(2 * a + m, 2 * b + n) for a, b in pairs for m, n in pols if listed(a, b, m, n)]
    inputs = np.array(inputs, np.int32)
    if order == "random":
        rs = np.random.RandomState(1)
        inputs = inputs[rs.permutation(len(inputs))]
        swap = (rs.random_sample(len(inputs)) < 0.5) & (inputs[:, 0] // 2 != inputs[:, 1] // 2)
        inputs[swap] = inputs[swap][:, ::-1]
    return np.ascontiguousarray(inputs)


def measure(channels, n_ant, order, rounds, calls):
    """One case in this process."""
    import numpy as np
    import torch  # (before the native library: one HIP runtime per process)

    from katsdpsigproc_amd import accel, hip
    from katsdpsigproc_amd.rfi import host, ingest

    class View:
        """A device buffer for ``torch.as_tensor``."""

        def __init__(self, array):
            self.__cuda_array_interface__ = {
                "shape": tuple(array.padded_shape), "typestr": array.dtype.str,
                "data": (array.buffer.ptr, False), "version": 2}  # fmt: skip

    def as_torch(array):
        t = torch.as_tensor(View(array), device="cuda")
        assert t.data_ptr() == array.buffer.ptr
        return t[:, : array.shape[1]]

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

    n_inputs = 2 * n_ant
    inputs = layout(n_ant, order)
    baselines = len(inputs)
    quad_antennas, quads = host.ApplyJonesHost.quad_table(inputs, n_inputs)
    n_quads = len(quads)
    samples = channels * baselines
    context = accel.create_some_context(interactive=False)
    # torch's current stream, so that one pair of events brackets any contender
    queue = hip.CommandQueue(context, stream=torch.cuda.current_stream().cuda_stream)
    template = ingest.ApplyJonesTemplate(context, flag_value=FLAG_VALUE)
    full = template.instantiate(queue, channels, baselines, n_inputs, n_quads)
    full.ensure_all_bound()
    kinds = ("vis", "weights", "flags")
    t = {name: as_torch(full.buffer(name)) for name in full.slots
         if name.replace("out_", "") in kinds}  # fmt: skip
    gen = torch.Generator(device="cuda").manual_seed(1)

    def rand(shape):
        return torch.rand(shape, generator=gen, device="cuda")

    for r0 in range(0, channels, 256):
        part = t["vis"][r0 : r0 + 256]
        part.copy_(torch.complex(rand(part.shape) - 0.5, rand(part.shape) - 0.5))
        t["weights"][r0 : r0 + 256].copy_(torch.exp2(rand(part.shape) * 6 - 3))
        t["flags"][r0 : r0 + 256].copy_((rand(part.shape) < 0.1).to(torch.uint8) * 3)
    rs = np.random.RandomState(2)
    shape = (channels, n_inputs)
    jones = np.zeros(shape + (2,), np.complex64)
    diagonal = rs.uniform(0.5, 1.5, shape) * np.exp(2j * np.pi * rs.random_sample(shape))
    leak = rs.uniform(0, 0.1, shape) * np.exp(2j * np.pi * rs.random_sample(shape))
    feed, rows_of = np.arange(n_inputs) % 2, np.arange(n_inputs)
    jones[:, rows_of, feed] = diagonal
    jones[:, rows_of, 1 - feed] = diagonal * leak
    jones[rs.random_sample(shape) < 0.01, 0] = complex(np.nan, 0.0)
    full.buffer("jones").set(queue, jones)
    full.buffer("quad_antennas").set(queue, quad_antennas)
    full.buffer("quads").set(queue, quads)
    torch.cuda.synchronize()
    rows = np.unique(np.random.RandomState(3).randint(0, channels, SAMPLED_ROWS))
    d_rows = torch.as_tensor(rows, device="cuda")
    kept = {name: t[name][d_rows].cpu().numpy() for name in kinds}
    want = host.ApplyJonesHost(FLAG_VALUE)(
        kept["vis"], jones[rows], quad_antennas, quads, kept["weights"], kept["flags"])  # fmt: skip

    def same(want, got, what):
        want, got = np.ascontiguousarray(want), np.ascontiguousarray(got)
        if want.dtype == np.uint8:
            assert np.array_equal(want, got), what
            return
        nan = np.isnan(want.view(np.float32))
        equal = want.view(np.uint32) == got.view(np.uint32)
        assert np.all(np.where(nan, np.isnan(got.view(np.float32)), equal)), what

    def restore():
        for name in kinds:
            t[name][d_rows] = torch.as_tensor(kept[name], device="cuda")

    # the composite's index tensors: the source of each entry (its mirror within a dish)
    t64 = quads.astype(np.int64)
    mirror = (t64 == 0) & (quad_antennas[:, :1] == quad_antennas[:, 1:])
    source = np.where(mirror, t64[:, [0, 2, 1, 3]], t64)
    assert (source != 0).all()
    conj = (source < 0) ^ mirror
    index = [torch.as_tensor(np.abs(source[:, e]) - 1, device="cuda") for e in range(4)]
    conj = [torch.as_tensor(conj[:, e], device="cuda") for e in range(4)]
    stored = [np.flatnonzero(t64[:, e] != 0) for e in range(4)]
    store_q = [torch.as_tensor(q, device="cuda") for q in stored]
    store_j = [torch.as_tensor(np.abs(t64[q, e]) - 1, device="cuda") for e, q in enumerate(stored)]
    store_conj = [torch.as_tensor(t64[q, e] < 0, device="cuda") for e, q in enumerate(stored)]
    ant = [torch.as_tensor(quad_antennas[:, k].astype(np.int64), device="cuda") for k in (0, 1)]
    d_jones = torch.as_tensor(jones, device="cuda").reshape(channels, n_ant, 2, 2)

    runs = []
    for in_place in (False, True):
        op = template.instantiate(queue, channels, baselines, n_inputs, n_quads)
        gains = ingest.ApplyGainsTemplate(context, flag_value=FLAG_VALUE).instantiate(
            queue, channels, baselines, n_inputs)  # fmt: skip
        for kind in kinds:
            bound = {kind: full.buffer(kind),
                     "out_" + kind: full.buffer(kind if in_place else "out_" + kind)}  # fmt: skip
            op.bind(**bound)
            gains.bind(**bound)
        op.bind(**{name: full.buffer(name) for name in ("jones", "quad_antennas", "quads")})
        # ApplyGains on the same arrays: one gain per input, the diagonal of its row
        gains.ensure_all_bound()
        gains.buffer("gains").set(queue, np.ascontiguousarray(jones[:, rows_of, feed]))
        gains.buffer("inputs").set(queue, inputs)
        out_vis = t["vis" if in_place else "out_vis"]

        def composite():
            v = t["vis"]
            s = [torch.where(conj[e], v.index_select(1, index[e]).conj(), v.index_select(1, index[e]))
                 for e in range(4)]  # fmt: skip
            coherency = torch.stack(s, dim=2).reshape(channels, n_quads, 2, 2)
            ca, cb = d_jones.index_select(1, ant[0]), d_jones.index_select(1, ant[1])
            product = (ca @ coherency @ cb.conj().transpose(2, 3)).reshape(channels, n_quads, 4)
            for e in range(4):
                o = product[:, :, e].index_select(1, store_q[e])
                out_vis.index_copy_(1, store_j[e], torch.where(store_conj[e], o.conj(), o))

        op()
        queue.finish()
        for kind, w in zip(kinds, want):
            same(w, t[kind if in_place else "out_" + kind][d_rows].cpu().numpy(), f"out_{kind}")
        restore()
        for _ in range(2):
            gains()
            composite()
            op()
        queue.finish()
        timed = time_rounds(queue, [op, gains, composite])
        restore()
        run = {"in_place": in_place, "op": timed[0], "apply_gains": timed[1],
               "torch_composite": timed[2]}  # fmt: skip
        total = samples * BYTES_PER_SAMPLE
        run["op"]["bytes_per_s"] = total / (timed[0]["median_ms"] * 1e-3)
        run["apply_gains"]["bytes_per_s"] = total / (timed[1]["median_ms"] * 1e-3)
        run["op_over_apply_gains"] = timed[0]["median_ms"] / timed[1]["median_ms"]
        run["torch_over_op"] = timed[2]["median_ms"] / timed[0]["median_ms"]
        runs.append(run)
    return {"device": context.device.name, "channels": channels, "antennas": n_ant,
            "order": order, "baselines": baselines, "n_quads": n_quads, "rounds": rounds,
            "calls": calls, "bytes": samples * BYTES_PER_SAMPLE, "verified": True, "runs": runs}  # fmt: skip


def text(entry):
    return f"{entry['median_ms']:.3f} ms ({entry['min_ms']:.3f}..{entry['max_ms']:.3f})"


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--case", action="append", help="CHANNELSxANTENNASxORDER (repeatable)")
    parser.add_argument("--rounds", type=int, default=5)
    parser.add_argument("--calls", type=int, default=10)
    parser.add_argument("--json")
    parser.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    args = parser.parse_args()
    cases = args.case or CASES
    if args.child:
        channels, n_ant, order = cases[0].split("x")
        print(json.dumps(measure(int(channels), int(n_ant), order, args.rounds, args.calls)))
        return
    results = []
    for case in cases:
        command = ["timeout", "-k", "10", str(CHILD_SECONDS), sys.executable,
                   os.path.abspath(__file__), "--child", "--case", case,
                   "--rounds", str(args.rounds), "--calls", str(args.calls)]  # fmt: skip
        done = subprocess.run(command, stdout=subprocess.PIPE, text=True)
        if done.returncode != 0:
            sys.exit(f"{case}: exit status {done.returncode}; nothing more is started")
        result = json.loads(done.stdout.strip().splitlines()[-1])
        print(f"{case} ({result['baselines']} baselines, {result['n_quads']} quads):")
        for run in result["runs"]:
            print(f"  {'in place    ' if run['in_place'] else 'out of place'}: op {text(run['op'])}, "
                  f"{run['op']['bytes_per_s'] / 1e12:.2f} TB/s; apply_gains "
                  f"{text(run['apply_gains'])}, {run['apply_gains']['bytes_per_s'] / 1e12:.2f} TB/s, "
                  f"op / apply_gains = {run['op_over_apply_gains']:.2f}; torch composite "
                  f"{text(run['torch_composite'])}, {run['torch_over_op']:.1f} x", flush=True)  # fmt: skip
        results.append(result)
    if args.json:
        with open(args.json, "w") as f:
            json.dump({"runs": results}, f, indent=1)


if __name__ == "__main__":
    main()
