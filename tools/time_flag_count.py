#!/usr/bin/env python3
"""Time the flag counter (``rfi.device.FlagCountTemplate``) against what torch can do on
the same device buffer.

Device time from events on one stream, data resident on the device, flag density 1/16, after
a warm-up; every figure is the median over ROUNDS rounds of CALLS calls (100 calls), with
the fastest and slowest round beside it as the run-to-run spread. Shapes: 4096 x 32768
(128 MiB: fits the 256 MiB Infinity Cache, so repeated calls are served from it) and
16384 x 32768 (512 MiB: read from HBM every call), channel-major and transposed, with 1
and 8 masks. The counts of every configuration are checked against NumPy outside the timed
region. The comparison, timed in alternation with the operation in the same rounds, is the
pair ``((t & m) != 0).sum(dim=k, dtype=torch.int32)``, k = 0 and 1, on a tensor that wraps
the operation's own ``flags`` buffer. Usage:
``python tools/time_flag_count.py [--rounds N] [--calls N] [--json OUT]``.
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

SHAPES = [(4096, 32768, "Infinity Cache"), (16384, 32768, "HBM")]
MASKS8 = (0xFF, 0x0F, 0xF0, 0x81, 0x80, 0x01, 0x7E, 0x18)
HBM_COPY_RATE = 6.3e12  # bytes/s, achievable


def make_flags(channels, baselines):
    """uint8 [channels][baselines], 1/16 of the bytes uniform in 1..255, drawn in blocks of
    rows (a fresh stream per block keeps the large shape cheap to make)."""
    out = np.zeros((channels, baselines), np.uint8)
    for r0 in range(0, channels, 512):
        rs = np.random.RandomState(r0 + 1)
        part = out[r0 : r0 + 512]
        hit = rs.random_sample(part.shape) < 1.0 / 16.0
        part[hit] = rs.randint(1, 256, int(np.count_nonzero(hit)))
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


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--rounds", type=int, default=5)
    parser.add_argument("--calls", type=int, default=20)
    parser.add_argument("--json")
    args = parser.parse_args()
    context = accel.create_some_context(interactive=False)
    # torch's current stream, so that one pair of events brackets either contender
    queue = hip.CommandQueue(context, stream=torch.cuda.current_stream().cuda_stream)
    result = {"device": context.device.name, "rounds": args.rounds, "calls": args.calls,
              "masks8": list(MASKS8), "density": 1.0 / 16.0, "runs": []}  # fmt: skip
    for channels, baselines, served_from in SHAPES:
        flags = make_flags(channels, baselines)
        want = host.FlagCountHost(MASKS8)(flags)
        print(f"{channels} x {baselines}: inputs and NumPy counts ready", flush=True)
        for transposed in (False, True):
            data = np.ascontiguousarray(flags.T) if transposed else flags
            for masks in ((0xFF,), MASKS8):
                op = device.FlagCountTemplate(context, masks, transposed=transposed).instantiate(
                    queue, channels, baselines)  # fmt: skip
                op.ensure_all_bound()
                op.buffer("flags").set(queue, data)
                op()  # warm-up, and the call that is checked
                n = len(masks)
                np.testing.assert_array_equal(want[0][:n], op.buffer("channel_counts").get(queue))
                np.testing.assert_array_equal(want[1][:n], op.buffer("baseline_counts").get(queue))
                run = {"channels": channels, "baselines": baselines, "transposed": transposed,
                       "masks": n, "served_from": served_from, "bytes": int(flags.size),
                       "verified": True}  # fmt: skip
                contenders = [op]
                if n == 1:
                    buf = op.buffer("flags")
                    t = torch.as_tensor(buf.buffer, device="cuda")[:, : data.shape[1]]
                    assert t.data_ptr() == buf.buffer.ptr and t.shape == data.shape

                    def torch_pair(t=t, m=masks[0]):
                        return (((t & m) != 0).sum(dim=0, dtype=torch.int32),
                                ((t & m) != 0).sum(dim=1, dtype=torch.int32))  # fmt: skip

                    over_rows, over_cols = (x.cpu().numpy() for x in torch_pair())
                    np.testing.assert_array_equal(want[0 if transposed else 1][0], over_rows)
                    np.testing.assert_array_equal(want[1 if transposed else 0][0], over_cols)
                    contenders.append(torch_pair)
                queue.finish()
                timed = time_rounds(queue, contenders, args.rounds, args.calls)
                run["op"] = timed[0]
                run["op"]["bytes_per_s"] = flags.size / (timed[0]["median_ms"] * 1e-3)
                run["op"]["share_of_hbm_copy_rate"] = run["op"]["bytes_per_s"] / HBM_COPY_RATE
                text = (f"  transposed={transposed!s:5} masks={n}: op {timed[0]['median_ms']:.4f} ms "
                        f"({timed[0]['min_ms']:.4f}..{timed[0]['max_ms']:.4f}), "
                        f"{run['op']['bytes_per_s'] / 1e12:.2f} TB/s [{served_from}]")  # fmt: skip
                if n == 1:
                    run["torch_pair"] = timed[1]
                    run["op_not_slower"] = timed[0]["median_ms"] <= timed[1]["median_ms"]
                    text += (f"; torch pair {timed[1]['median_ms']:.4f} ms "
                             f"({timed[1]['min_ms']:.4f}..{timed[1]['max_ms']:.4f})")  # fmt: skip
                print(text, flush=True)
                result["runs"].append(run)
                del op
            del data
    if args.json:
        with open(args.json, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
