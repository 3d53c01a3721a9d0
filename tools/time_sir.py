#!/usr/bin/env python3
"""Time the scale-invariant rank flag extension (``rfi.device.ScaleInvariantRankTemplate``)
against what a caller could do without it, and against a single read of the same bytes.

Device time from events on one stream, data resident on the device, after a warm-up; every
figure is the median over ROUNDS rounds of CALLS calls, with the fastest and slowest round
beside it as the run-to-run spread. Shapes: 4096 x 32768 (128 MiB: fits the 256 MiB Infinity
Cache) and 16384 x 32768 (512 MiB: from HBM every call), channel-major and transposed. Flags:
density 1/16 plus bursts of 1..200 channels, in bit 0; the operation reads bit 0 and writes
bit 1 (``mask=1, flag_value=2``), so every call sees the same input and does the same work.
The result is checked against ``rfi.host.ScaleInvariantRankHost`` on sampled baselines.

Timed in alternation with the operation, in the same rounds:

* the torch composite on a tensor that wraps the operation's own ``flags`` buffer: int32
  ``cumsum``, ``cummin``, flipped ``cummax``, compare, OR (its result is checked too);
* ``rfi.device.FlagCount`` with one mask on the same buffer: one read pass over the same
  bytes, the streaming floor. The operator reads the flags two to three times and writes
  them once.

Usage: ``python tools/time_sir.py [--rounds N] [--calls N] [--shapes small|large|all]
[--json OUT]``.
"""

import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402  (before the native library: one HIP runtime per process)

from katsdpsigproc_amd import accel, hip  # noqa: E402
from katsdpsigproc_amd.rfi import device, host  # noqa: E402

SHAPES = {"small": (4096, 32768, "Infinity Cache"), "large": (16384, 32768, "HBM")}
ETA = 0.2
MASK, FLAG_VALUE = 1, 2
SAMPLED_BASELINES = 96


def make_flags(channels, baselines):
    """uint8 [channels][baselines]: bit 0 set on 1/16 of the samples, and on 4 bursts of
    1..200 channels per 64 baselines; drawn in blocks of rows."""
    out = np.zeros((channels, baselines), np.uint8)
    for r0 in range(0, channels, 512):
        rs = np.random.RandomState(r0 + 1)
        part = out[r0 : r0 + 512]
        part[rs.random_sample(part.shape) < 1.0 / 16.0] = 1
    rs = np.random.RandomState(7)
    for b in rs.randint(0, baselines, baselines // 16):
        length = int(rs.randint(1, 201))
        start = int(rs.randint(0, channels - length + 1))
        out[start : start + length, b] = 1
    return out


def time_rounds(queue, functions, rounds, calls):
    """Seconds per call of each function: rounds x calls, the functions taking turns."""
    times = [[] for _ in functions]
    for _ in range(rounds):
        for i, fn in enumerate(functions):
            start = queue.enqueue_marker()
            for _ in range(calls):
                fn()
            stop = queue.enqueue_marker()
            times[i].append(stop.time_since(start) / calls)
    return [{"median_ms": float(np.median(t)) * 1e3, "min_ms": min(t) * 1e3, "max_ms": max(t) * 1e3}
            for t in times]  # fmt: skip


def torch_sir(t, dim, eta_q):
    """The composite a caller can write with torch alone, in place on uint8 `t`."""
    n = t.shape[dim]
    flagged = (t & MASK) != 0
    psi = flagged.to(torch.int32) * 4096 + (eta_q - 4096)
    zero_shape = list(t.shape)
    zero_shape[dim] = 1
    m = torch.cat([torch.zeros(zero_shape, dtype=torch.int32, device=t.device),
                   torch.cumsum(psi, dim=dim, dtype=torch.int32)], dim=dim)  # fmt: skip
    lowest = torch.cummin(m.narrow(dim, 0, n), dim=dim).values
    highest = torch.cummax(m.narrow(dim, 1, n).flip(dim), dim=dim).values.flip(dim)
    t |= (highest >= lowest).to(torch.uint8) * FLAG_VALUE


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--rounds", type=int, default=5)
    parser.add_argument("--calls", type=int, default=10)
    parser.add_argument("--shapes", choices=["small", "large", "all"], default="all")
    parser.add_argument("--json")
    args = parser.parse_args()
    context = accel.create_some_context(interactive=False)
    # torch's current stream, so that one pair of events brackets any contender
    queue = hip.CommandQueue(context, stream=torch.cuda.current_stream().cuda_stream)
    reference = host.ScaleInvariantRankHost(ETA, MASK, FLAG_VALUE)
    result = {"device": context.device.name, "rounds": args.rounds, "calls": args.calls,
              "eta_q": reference.eta_q, "density": 1.0 / 16.0, "runs": []}  # fmt: skip
    names = ["small", "large"] if args.shapes == "all" else [args.shapes]
    for channels, baselines, served_from in (SHAPES[name] for name in names):
        flags = make_flags(channels, baselines)
        sample = np.unique(np.random.RandomState(3).randint(0, baselines, SAMPLED_BASELINES))
        want = reference(np.ascontiguousarray(flags[:, sample]))
        assert (want != flags[:, sample]).any()
        print(f"{channels} x {baselines}: inputs and NumPy reference ready", flush=True)
        for transposed in (False, True):
            data = np.ascontiguousarray(flags.T) if transposed else flags
            op = device.ScaleInvariantRankTemplate(
                context, ETA, MASK, FLAG_VALUE, transposed=transposed).instantiate(
                queue, channels, baselines)  # fmt: skip
            op.ensure_all_bound()
            buf = op.buffer("flags")
            count = device.FlagCountTemplate(context, (MASK,), transposed=transposed).instantiate(
                queue, channels, baselines)  # fmt: skip
            count.bind(flags=buf)
            count.ensure_all_bound()
            t = torch.as_tensor(buf.buffer, device="cuda")[:, : data.shape[1]]
            assert t.data_ptr() == buf.buffer.ptr and t.shape == data.shape
            dim = 1 if transposed else 0

            def sampled():
                got = buf.get(queue)
                return got[sample].T if transposed else got[:, sample]

            # the composite first, checked, then the input again for the operation
            buf.set(queue, data)
            torch_sir(t, dim, reference.eta_q)
            torch.cuda.synchronize()
            np.testing.assert_array_equal(want, sampled())
            buf.set(queue, data)
            op()  # warm-up, and the call that is checked
            np.testing.assert_array_equal(want, sampled())
            count()
            queue.finish()
            timed = time_rounds(queue, [op, lambda: torch_sir(t, dim, reference.eta_q), count],
                                args.rounds, args.calls)  # fmt: skip
            np.testing.assert_array_equal(want, sampled())  # still the same after all calls
            run = {"channels": channels, "baselines": baselines, "transposed": transposed,
                   "served_from": served_from, "bytes": int(flags.size), "verified": True,
                   "op": timed[0], "torch_composite": timed[1], "flag_count": timed[2]}  # fmt: skip
            run["torch_over_op"] = timed[1]["median_ms"] / timed[0]["median_ms"]
            run["op_over_flag_count"] = timed[0]["median_ms"] / timed[2]["median_ms"]
            run["op"]["bytes_per_s"] = flags.size / (timed[0]["median_ms"] * 1e-3)
            print(f"  transposed={transposed!s:5}: op {timed[0]['median_ms']:.4f} ms "
                  f"({timed[0]['min_ms']:.4f}..{timed[0]['max_ms']:.4f}); torch composite "
                  f"{timed[1]['median_ms']:.3f} ms ({timed[1]['min_ms']:.3f}..{timed[1]['max_ms']:.3f}), "
                  f"{run['torch_over_op']:.1f} x; FlagCount {timed[2]['median_ms']:.4f} ms "
                  f"({timed[2]['min_ms']:.4f}..{timed[2]['max_ms']:.4f}), op = "
                  f"{run['op_over_flag_count']:.2f} x [{served_from}]", flush=True)  # fmt: skip
            result["runs"].append(run)
            del op, count, t, buf
            torch.cuda.empty_cache()
        del flags
    if args.json:
        with open(args.json, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
