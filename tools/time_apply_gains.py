#!/usr/bin/env python3
"""Time the application of gains (``rfi.ingest.ApplyGainsTemplate``) against what a caller
could do without it, and against a streaming kernel.

Device time from events on one stream, data resident on the device, after a warm-up; every
figure is the median over ROUNDS rounds of CALLS calls, with the fastest and slowest round
beside it as the run-to-run spread. Shapes: 4096 x 32768 with 256 inputs (3.25 GiB of samples
in and out: from HBM every call) and 4096 x 2016 with 128 inputs (210 MiB, which fits the
Infinity Cache). The baselines are the pairs a <= b of the inputs in order, so neighbouring
baselines share an input; the gains have magnitudes around 1 and 1 % NaN. All four variants
(weights, flags), out of place and in place. The result of the warm-up call is compared with
``rfi.host.ApplyGainsHost`` on sampled rows, bit for bit (a NaN for a NaN).

Timed in alternation with the operation, in the same rounds:

* the torch composite a caller can write today on tensors that wrap the operation's own
  buffers: ``index_select`` of the gains twice, a complex multiply for the correction and one
  for the visibilities, and the weight and flag expressions (not bit for bit the definition:
  torch's complex multiply rounds as it likes);
* the float32 transpose of the same shape, which reads 4 and writes 4 bytes per sample, as the
  yardstick for streaming speed; the operation reads and writes 8 (vis) + 4 (weights) +
  1 (flags) bytes per sample, 26 with everything.

Every shape is measured in a process of its own, started under a time limit; the first one
that fails ends the run.

Usage: ``python tools/time_apply_gains.py [--rounds N] [--calls N] [--json OUT]
[--shape CxBxN ...]``.
"""

import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = ["4096x32768x256", "4096x2016x128"]
SAMPLED_ROWS = 6
CHILD_SECONDS = 300
FLAG_VALUE = 128


def measure(channels, baselines, n_inputs, rounds, calls):
    """One shape, every variant, in this process."""
    import numpy as np
    import torch  # (before the native library: one HIP runtime per process)

    from katsdpsigproc_amd import accel, hip, transpose
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

    samples = channels * baselines
    context = accel.create_some_context(interactive=False)
    # torch's current stream, so that one pair of events brackets any contender
    queue = hip.CommandQueue(context, stream=torch.cuda.current_stream().cuda_stream)
    # the full operation owns the buffers; the other variants bind the same ones
    full = ingest.ApplyGainsTemplate(context, flag_value=FLAG_VALUE).instantiate(
        queue, channels, baselines, n_inputs)  # fmt: skip
    full.ensure_all_bound()
    t = {name: as_torch(full.buffer(name)) for name in full.slots}
    gen = torch.Generator(device="cuda").manual_seed(1)

    def rand(shape):
        return torch.rand(shape, generator=gen, device="cuda")

    for r0 in range(0, channels, 256):
        part = t["vis"][r0 : r0 + 256]
        part.copy_(torch.complex(rand(part.shape) - 0.5, rand(part.shape) - 0.5))
        t["weights"][r0 : r0 + 256].copy_(torch.exp2(rand(part.shape) * 6 - 3))
        t["flags"][r0 : r0 + 256].copy_((rand(part.shape) < 0.1).to(torch.uint8) * 3)
    shape = (channels, n_inputs)
    gains = torch.polar(0.5 + rand(shape), rand(shape) * 6.2831853)
    gains.masked_fill_(rand(shape) < 0.01, complex(float("nan"), 0.0))
    t["gains"].copy_(gains)
    pairs = np.array([(a, b) for a in range(n_inputs) for b in range(a, n_inputs)], np.int32)
    inputs = np.ascontiguousarray(np.resize(pairs, (baselines, 2)))
    full.buffer("inputs").set(queue, inputs)
    a, b = (torch.as_tensor(inputs[:, k].astype(np.int64), device="cuda") for k in (0, 1))
    yardstick = transpose.TransposeTemplate(context, np.float32, "float").instantiate(
        queue, (channels, baselines))  # fmt: skip
    yardstick.ensure_all_bound()
    as_torch(yardstick.buffer("src")).copy_(t["weights"])
    torch.cuda.synchronize()
    rows = np.unique(np.random.RandomState(3).randint(0, channels, SAMPLED_ROWS))
    d_rows = torch.as_tensor(rows, device="cuda")
    kept = {name: t[name][d_rows].cpu().numpy() for name in ("vis", "weights", "flags", "gains")}

    def same(want, got, what):
        want, got = np.ascontiguousarray(want), np.ascontiguousarray(got)
        if want.dtype == np.uint8:
            assert np.array_equal(want, got), what
            return
        nan = np.isnan(want.view(np.float32))
        equal = want.view(np.uint32) == got.view(np.uint32)
        assert np.all(np.where(nan, np.isnan(got.view(np.float32)), equal)), what

    def restore():
        for name in ("vis", "weights", "flags"):
            t[name][d_rows] = torch.as_tensor(kept[name], device="cuda")

    runs = []
    for weights in (True, False):
        for flags in (True, False):
            kinds = ["vis"] + (["weights"] if weights else []) + (["flags"] if flags else [])
            want = host.ApplyGainsHost(FLAG_VALUE)(
                kept["vis"], kept["gains"], inputs, kept["weights"] if weights else None,
                kept["flags"] if flags else None)  # fmt: skip
            template = ingest.ApplyGainsTemplate(context, weights=weights, flags=flags,
                                                 flag_value=FLAG_VALUE)  # fmt: skip
            for in_place in (False, True):
                op = template.instantiate(queue, channels, baselines, n_inputs)
                for kind in kinds:
                    op.bind(**{kind: full.buffer(kind),
                               "out_" + kind: full.buffer(kind if in_place else "out_" + kind)})
                op.bind(gains=full.buffer("gains"), inputs=full.buffer("inputs"))
                out = {kind: t[kind if in_place else "out_" + kind] for kind in kinds}

                def composite():
                    g = t["gains"]
                    c = g.index_select(1, a) * g.index_select(1, b).conj()
                    ok = ~(c.real.isnan() | c.imag.isnan())
                    out["vis"].copy_(torch.where(ok, t["vis"] * c, t["vis"]))
                    if weights:
                        p = c.real * c.real + c.imag * c.imag
                        out["weights"].copy_(torch.where(ok & (p > 0), t["weights"] / p, 0.0))
                    if flags:
                        bit = torch.where(ok, 0, FLAG_VALUE).to(torch.uint8)
                        out["flags"].copy_(t["flags"] | bit)

                op()
                queue.finish()
                for kind, w in zip(("vis", "weights", "flags"), want):
                    if kind in kinds:
                        same(w, out[kind][d_rows].cpu().numpy(), f"out_{kind}")
                restore()
                for _ in range(2):
                    yardstick()
                    composite()
                    op()
                queue.finish()
                timed = time_rounds(queue, [op, composite, yardstick])
                restore()
                per_sample = 16 + (8 if weights else 0) + (2 if flags else 0)
                run = {"weights": weights, "flags": flags, "in_place": in_place,
                       "bytes_per_sample": per_sample, "bytes": samples * per_sample,
                       "op": timed[0], "torch_composite": timed[1], "transpose": timed[2]}  # fmt: skip
                run["op"]["bytes_per_s"] = samples * per_sample / (timed[0]["median_ms"] * 1e-3)
                run["transpose"]["bytes_per_s"] = samples * 8 / (timed[2]["median_ms"] * 1e-3)
                run["torch_over_op"] = timed[1]["median_ms"] / timed[0]["median_ms"]
                # against the time the transpose's rate would need for this variant's bytes
                run["op_over_transpose_at_same_bytes"] = timed[0]["median_ms"] / (
                    timed[2]["median_ms"] * per_sample / 8)
                runs.append(run)
    return {"device": context.device.name, "channels": channels, "baselines": baselines,
            "n_inputs": n_inputs, "rounds": rounds, "calls": calls, "verified": True,
            "variants": runs}  # fmt: skip


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
        result = json.loads(done.stdout.strip().splitlines()[-1])
        print(f"{shape}:")
        for run in result["variants"]:
            print(f"  weights {run['weights']:d} flags {run['flags']:d} "
                  f"{'in place    ' if run['in_place'] else 'out of place'}: op {text(run['op'])}, "
                  f"{run['op']['bytes_per_s'] / 1e12:.2f} TB/s; torch composite "
                  f"{text(run['torch_composite'])}, {run['torch_over_op']:.1f} x; transpose "
                  f"{text(run['transpose'])}, {run['transpose']['bytes_per_s'] / 1e12:.2f} TB/s; "
                  f"op / (transpose at the same bytes) = "
                  f"{run['op_over_transpose_at_same_bytes']:.2f}", flush=True)  # fmt: skip
        results.append(result)
    if args.json:
        with open(args.json, "w") as f:
            json.dump({"runs": results}, f, indent=1)


if __name__ == "__main__":
    main()
