#!/usr/bin/env python3
"""Time the masked Gaussian filter's device operation (``rfi.twodflag.MaskedGaussianFilter``).

Device time from events, after a warm-up call, data resident on the device, float32,
4 passes, sigma (12.5, 10) -- the 2-D flagger's default background (box radii 10 and 8) --
at the flagger's per-batch shapes 178 x (100 x 4096) and 56 x (32 x 32768) and for one
4096 x 4096 image. Each shape is timed whole and with either axis alone. Usage:
``python tools/time_masked_filter.py [--reps N] [--dtype float32|float64] [--json OUT]``.
Under ``rocprofv3 --kernel-trace --stats`` the same run gives the time of each ``mf_*`` kernel.
"""

import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from katsdpsigproc_amd import accel  # noqa: E402
from katsdpsigproc_amd.rfi import twodflag  # noqa: E402

SHAPES = [(178, 100, 4096), (56, 32, 32768), (1, 4096, 4096)]
SIGMA = (12.5, 10.0)


def time_shape(context, queue, shape, dtype, reps):
    rs = np.random.RandomState(1)
    data = (2.0 + 0.1 * rs.standard_normal(shape)).astype(dtype)
    flags = (rs.uniform(size=shape) < 0.05).astype(np.uint8)
    template = twodflag.MaskedGaussianFilterTemplate(context, dtype, 4)
    out = {"shape": list(shape), "dtype": np.dtype(dtype).name}
    for label, sigma in (("both", SIGMA), ("axis0", (SIGMA[0], 0.0)), ("axis1", (0.0, SIGMA[1]))):
        op = template.instantiate(queue, shape, sigma)
        op.ensure_all_bound()
        op.buffer("data").set(queue, data)
        op.buffer("flags").set(queue, flags)
        op()
        queue.finish()
        start = queue.enqueue_marker()
        for _ in range(reps):
            op()
        stop = queue.enqueue_marker()
        ms = stop.time_since(start) / reps * 1e3
        out[label] = {"radii": list(op.radii), "batch": op.batch,
                      "workspace_bytes": op.workspace_bytes, "ms_per_call": ms,
                      "ms_per_image": ms / shape[0],
                      "nan_fraction": float(np.isnan(op.buffer("out").get(queue)).mean())}  # fmt: skip
        del op
    return out


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--reps", type=int, default=3)
    parser.add_argument("--dtype", default="float32", choices=["float32", "float64"])
    parser.add_argument("--json")
    args = parser.parse_args()
    context = accel.create_some_context(interactive=False)
    queue = context.create_command_queue()
    result = {"device": context.device.name, "sigma": list(SIGMA), "passes": 4, "runs": []}
    for shape in SHAPES:
        r = time_shape(context, queue, shape, np.dtype(args.dtype), args.reps)
        result["runs"].append(r)
        print(f"{r['shape']} {r['dtype']}: " + ", ".join(
            f"{k} {r[k]['ms_per_call']:.2f} ms ({r[k]['ms_per_image']:.3f} per image)"
            for k in ("both", "axis0", "axis1")), flush=True)  # fmt: skip
    if args.json:
        with open(args.json, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
