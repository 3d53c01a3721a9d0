#!/usr/bin/env python3
"""Time the compression of weights (``rfi.ingest.CompressWeightsTemplate``) against what a
caller could do without it, and against a streaming kernel.

Device time from events on one stream, data resident on the device, after a warm-up; every
figure is the median over ROUNDS rounds of CALLS calls, with the fastest and slowest round
beside it as the run-to-run spread. Shapes: 4096 x 32768 (weights of 512 MiB: from HBM every
call) and 512 x 32768 (what ``channel_factor=8`` leaves of it: 64 MiB, which fits the
Infinity Cache). Weights are 2^U(-3, 3) with 10 % zeros. The result of the warm-up call is
compared with ``rfi.host.CompressWeightsHost`` on sampled rows, bit for bit.

Timed in alternation with the operation, in the same rounds:

* the torch composite a caller can write today on tensors that wrap the operation's own
  buffers: a masked ``amax``, a divide, ``round``, ``clamp``, a compare and a cast (its bytes
  are checked to differ from the definition's by at most 1: torch's division is not correctly
  rounded);
* the float32 transpose of the same shape, which reads 4 and writes 4 bytes per sample, as the
  yardstick for streaming speed; the operation reads 4 and writes 1.

Every shape is measured in a process of its own, started under a time limit; the first one
that fails ends the run.

Usage: ``python tools/time_compress_weights.py [--rounds N] [--calls N] [--json OUT]
[--shape CxB ...]``.
"""

import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = ["4096x32768", "512x32768"]
SAMPLED_ROWS = 8
CHILD_SECONDS = 240


def measure(channels, baselines, rounds, calls):
    """One shape, in this process."""
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
        return t[:, : array.shape[1]] if len(array.shape) == 2 else t[: array.shape[0]]

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
    op = ingest.CompressWeightsTemplate(context).instantiate(queue, channels, baselines)
    op.ensure_all_bound()
    t = {name: as_torch(op.buffer(name)) for name in op.slots}
    gen = torch.Generator(device="cuda").manual_seed(1)
    for r0 in range(0, channels, 256):
        part = t["weights"][r0 : r0 + 256]
        part.copy_(torch.exp2(torch.rand(part.shape, generator=gen, device="cuda") * 6 - 3))
        part.masked_fill_(torch.rand(part.shape, generator=gen, device="cuda") < 0.1, 0.0)
    torch.cuda.synchronize()
    rows = torch.as_tensor(np.unique(np.random.RandomState(3).randint(0, channels, SAMPLED_ROWS)),
                           device="cuda")  # fmt: skip
    want8, want_wc = host.CompressWeightsHost()(t["weights"][rows].cpu().numpy())

    def composite():
        w = t["weights"]
        ok = (w > 0) & (w < float("inf"))
        wc = torch.where(ok, w, 0.0).amax(dim=1) / 255.0
        q = (w / wc.unsqueeze(1)).round().clamp(1.0, 255.0)
        t["weights8"].copy_(torch.where(w > 0, q, 0.0).to(torch.uint8))
        t["weights_channel"].copy_(wc)

    composite()
    torch.cuda.synchronize()
    got8 = t["weights8"][rows].cpu().numpy().astype(np.int32)
    assert np.abs(got8 - want8).max() <= 1, "the torch composite is off by more than 1"
    composite_mismatches = int(np.count_nonzero(got8 != want8))
    t["weights8"].zero_()
    t["weights_channel"].zero_()
    op()
    queue.finish()
    np.testing.assert_array_equal(t["weights8"][rows].cpu().numpy(), want8)
    np.testing.assert_array_equal(t["weights_channel"][rows].cpu().numpy().view(np.uint32),
                                  want_wc.view(np.uint32))  # fmt: skip
    yardstick = transpose.TransposeTemplate(context, np.float32, "float").instantiate(
        queue, (channels, baselines))  # fmt: skip
    yardstick.ensure_all_bound()
    as_torch(yardstick.buffer("src")).copy_(t["weights"])
    for _ in range(3):
        yardstick()
        op()
    queue.finish()
    timed = time_rounds(queue, [op, composite, yardstick])
    op_bytes = samples * 5 + channels * 4
    run = {"device": context.device.name, "channels": channels, "baselines": baselines,
           "rounds": rounds, "calls": calls, "verified": True, "bytes": int(op_bytes),
           "composite_bytes_off_by_one": composite_mismatches, "op": timed[0],
           "torch_composite": timed[1], "transpose": timed[2],
           "transpose_bytes": int(samples * 8)}  # fmt: skip
    run["op"]["bytes_per_s"] = op_bytes / (timed[0]["median_ms"] * 1e-3)
    run["transpose"]["bytes_per_s"] = samples * 8 / (timed[2]["median_ms"] * 1e-3)
    run["torch_over_op"] = timed[1]["median_ms"] / timed[0]["median_ms"]
    # the time the transpose's rate would need for this operation's 5 bytes per sample
    run["op_over_transpose_at_5_bytes"] = timed[0]["median_ms"] / (timed[2]["median_ms"] * 5 / 8)
    return run


def text(entry):
    return f"{entry['median_ms']:.3f} ms ({entry['min_ms']:.3f}..{entry['max_ms']:.3f})"


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--shape", action="append", help="CHANNELSxBASELINES (repeatable)")
    parser.add_argument("--rounds", type=int, default=5)
    parser.add_argument("--calls", type=int, default=10)
    parser.add_argument("--json")
    parser.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    args = parser.parse_args()
    shapes = args.shape or SHAPES
    if args.child:
        channels, baselines = (int(n) for n in shapes[0].split("x"))
        print(json.dumps(measure(channels, baselines, args.rounds, args.calls)))
        return
    runs = []
    for shape in shapes:
        command = ["timeout", "-k", "10", str(CHILD_SECONDS), sys.executable,
                   os.path.abspath(__file__), "--child", "--shape", shape,
                   "--rounds", str(args.rounds), "--calls", str(args.calls)]  # fmt: skip
        done = subprocess.run(command, stdout=subprocess.PIPE, text=True)
        if done.returncode != 0:
            sys.exit(f"{shape}: exit status {done.returncode}; nothing more is started")
        run = json.loads(done.stdout.strip().splitlines()[-1])
        print(f"  {shape}: op {text(run['op'])}, {run['op']['bytes_per_s'] / 1e12:.2f} TB/s; "
              f"torch composite {text(run['torch_composite'])}, {run['torch_over_op']:.1f} x; "
              f"transpose {text(run['transpose'])}, "
              f"{run['transpose']['bytes_per_s'] / 1e12:.2f} TB/s; op / (transpose at 5 bytes "
              f"per sample) = {run['op_over_transpose_at_5_bytes']:.2f}", flush=True)  # fmt: skip
        runs.append(run)
    if args.json:
        with open(args.json, "w") as f:
            json.dump({"runs": runs}, f, indent=1)


if __name__ == "__main__":
    main()
