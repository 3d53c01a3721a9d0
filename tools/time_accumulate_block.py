#!/usr/bin/env python3
"""Time one launch of ``rfi.ingest.AccumulateBlock`` over D dumps against D launches of
``rfi.device.Accumulate`` on the same buffers, for D in {2, 4, 8}.

Device time from event pairs on one stream, data resident on the device, after a warm-up.
Shape 4096 x 32768 by default, with weights and without a mask: the accumulators alone are
1.6 GiB and a dump is 1.6 GiB, far beyond the 256 MiB Infinity Cache, so every call streams
from and to HBM. 1/16 of the samples are flagged. The contenders take turns within one
session: a round times, for each D, the block launch and then the D single launches (one
event pair around all D, which the stream runs back to back), and every figure is the median
of the rounds with the fastest and the slowest round beside it. The yardstick of a block of D
is always the D single launches of the same round, never the block kernel at another D.

Bytes are what the launches must move, computed from the shape: 39 per sample and dump for the
single launches (8 vis + 1 flags + 4 weights in, 13 of accumulators in and out), 13 D + 26 for
a block. The first and last 8 rows of the accumulators after a block are checked against
``rfi.host.AveragerHost`` outside the timed region, and the block and the single launches must
leave the same accumulators everywhere, bit for bit. Usage:
``python tools/time_accumulate_block.py [--channels C] [--baselines B] [--rounds N] [--json OUT]``.
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
from katsdpsigproc_amd.rfi import device, host, ingest  # noqa: E402

EDGE = 8  # rows checked at either end
ACC = ("acc_vis", "acc_weights", "acc_flags")
BLOCKS = (2, 4, 8)


class _View:
    """A device buffer under another element type, for ``torch.as_tensor``."""

    def __init__(self, buffer, shape, typestr):
        self.__cuda_array_interface__ = {"shape": tuple(shape), "typestr": typestr,
                                         "data": (buffer.ptr, False), "version": 2}  # fmt: skip


def as_torch(array):
    """Tensor over the data of a 2-D DeviceArray (padding sliced off); complex64 comes as
    float32 with a last axis of 2."""
    shape, padded = array.shape, array.padded_shape
    if array.dtype == np.complex64:
        t = torch.as_tensor(_View(array.buffer, padded + (2,), "<f4"), device="cuda")
    else:
        t = torch.as_tensor(_View(array.buffer, padded, array.dtype.str), device="cuda")
    assert t.data_ptr() == array.buffer.ptr
    return t[: shape[0], : shape[1]]


def edge_rows(t):
    """First and last EDGE rows of a tensor as one NumPy array."""
    a = torch.cat([t[:EDGE], t[-EDGE:]]).cpu().numpy()
    return a.view(np.complex64)[..., 0] if a.ndim == 3 else a


def same(want, got, what):
    want = np.ascontiguousarray(want)
    got = np.ascontiguousarray(got)
    if want.dtype != np.uint8:
        want, got = want.view(np.float32), got.view(np.float32)
        ok = (want.view(np.uint32) == got.view(np.uint32)) | (np.isnan(want) & np.isnan(got))
    else:
        ok = want == got
    if not ok.all():
        raise AssertionError(f"{what}: {np.count_nonzero(~ok)} of {ok.size} values differ")


def summary(times):
    return {"median_ms": float(np.median(times)), "min_ms": min(times), "max_ms": max(times)}


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--channels", type=int, default=4096)
    parser.add_argument("--baselines", type=int, default=32768)
    parser.add_argument("--rounds", type=int, default=20)
    parser.add_argument("--json")
    args = parser.parse_args()
    channels, baselines, rounds = args.channels, args.baselines, args.rounds
    samples = channels * baselines
    dumps = max(BLOCKS)
    context = accel.create_some_context(interactive=False)
    # torch's current stream, so that the fills and the launches are in one order
    queue = hip.CommandQueue(context, stream=torch.cuda.current_stream().cuda_stream)
    gen = torch.Generator(device="cuda").manual_seed(1)

    block = ingest.AccumulateBlockTemplate(context, dumps).instantiate(queue, channels, baselines)
    block.ensure_all_bound()
    for d in range(dumps):
        vis, flags, weights = (as_torch(block.buffer(f"{kind}{d}")) for kind in ("vis", "flags", "weights"))
        vis.copy_(torch.randn(vis.shape, generator=gen, device="cuda"))
        hit = torch.rand(flags.shape, generator=gen, device="cuda") < 1.0 / 16.0
        flags.copy_(torch.randint(1, 256, flags.shape, generator=gen, device="cuda",
                                  dtype=torch.uint8) * hit)  # fmt: skip
        weights.copy_(torch.rand(weights.shape, generator=gen, device="cuda") * 1.5 + 0.5)
        del vis, flags, weights, hit
    # the existing operation, once per dump, on the block's buffers
    singles = []
    for d in range(dumps):
        op = device.AccumulateTemplate(context).instantiate(queue, channels, baselines)
        op.bind(vis=block.buffer(f"vis{d}"), flags=block.buffer(f"flags{d}"),
                weights=block.buffer(f"weights{d}"), **{name: block.buffer(name) for name in ACC})  # fmt: skip
        singles.append(op)
    acc = {name: as_torch(block.buffer(name)) for name in ACC}

    def clear_acc():
        for name in ACC:
            block.buffer(name).zero(queue)

    def run_block(n):
        block.n_dumps = n
        block()

    def run_singles(n):
        for op in singles[:n]:
            op()

    # ------------------------------------------------------- verification and warm-up
    for n in BLOCKS:
        clear_acc()
        run_block(n)
        reference = host.AveragerHost(2 * EDGE, baselines)
        for d in range(n):
            reference.add(*(edge_rows(as_torch(block.buffer(f"{kind}{d}")))
                            for kind in ("vis", "flags", "weights")))  # fmt: skip
        for name, want in zip(ACC, (reference.acc_vis, reference.acc_weights, reference.acc_flags)):
            same(want, edge_rows(acc[name]), f"{name} after a block of {n}")
        after_block = {name: acc[name].clone() for name in ACC}
        clear_acc()
        run_singles(n)
        for name in ACC:
            if not torch.equal(after_block[name].contiguous().view(torch.uint8),
                               acc[name].contiguous().view(torch.uint8)):
                raise AssertionError(f"{name}: a block of {n} and {n} launches differ")
        del after_block
    torch.cuda.empty_cache()
    queue.finish()

    # ------------------------------------------------------------------------ timing
    times = {n: {"block": [], "singles": []} for n in BLOCKS}
    for _ in range(rounds):
        for n in BLOCKS:
            for contender, fn in (("block", run_block), ("singles", run_singles)):
                start = queue.enqueue_marker()
                fn(n)
                stop = queue.enqueue_marker()
                times[n][contender].append(stop.time_since(start) * 1e3)
    result = {"device": context.device.name, "channels": channels, "baselines": baselines,
              "rounds": rounds, "density": 1.0 / 16.0, "verified": True, "blocks": []}  # fmt: skip
    print(f"{context.device.name}, {channels} x {baselines}, weights, no mask, {rounds} rounds; "
          "median ms (fastest..slowest)", flush=True)  # fmt: skip
    for n in BLOCKS:
        one, many = summary(times[n]["block"]), summary(times[n]["singles"])
        block_bytes, singles_bytes = samples * (13 * n + 26), samples * 39 * n
        for entry, n_bytes in ((one, block_bytes), (many, singles_bytes)):
            entry["bytes"] = int(n_bytes)
            entry["bytes_per_s"] = n_bytes / (entry["median_ms"] * 1e-3)
        spread = max(one["max_ms"] - one["min_ms"], many["max_ms"] - many["min_ms"])
        run = {"dumps": n, "block": one, "singles": many,
               "byte_ratio": block_bytes / singles_bytes,
               "time_ratio": one["median_ms"] / many["median_ms"],
               "gain_ms": many["median_ms"] - one["median_ms"], "spread_ms": spread,
               "faster_by_more_than_the_spread": many["median_ms"] - one["median_ms"] > spread}  # fmt: skip
        result["blocks"].append(run)
        print(f"  D={n}: block {one['median_ms']:.3f} ({one['min_ms']:.3f}..{one['max_ms']:.3f}), "
              f"{one['bytes_per_s'] / 1e12:.2f} TB/s; {n} launches {many['median_ms']:.3f} "
              f"({many['min_ms']:.3f}..{many['max_ms']:.3f}), {many['bytes_per_s'] / 1e12:.2f} TB/s; "
              f"time ratio {run['time_ratio']:.3f}, byte ratio {run['byte_ratio']:.3f}, "
              f"gain {run['gain_ms']:.3f} ms against a spread of {spread:.3f} ms", flush=True)  # fmt: skip
    if args.json:
        with open(args.json, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
