#!/usr/bin/env python3
"""Time the range percentiles (``rfi.ingest.RangePercentilesTemplate``) against the eight
``Percentile5`` operations they replace, and against a streaming kernel.

Device time from events on one stream, data resident on the device, after a warm-up; every
figure is the median over ROUNDS rounds of CALLS calls, with the fastest and slowest round
beside it as the run-to-run spread. Shapes: 4096 x 8320 complex64 (272 MB: from HBM every call)
and 512 x 8320 (what ``channel_factor=8`` leaves of it, which fits the Infinity Cache). The
ranges are the eight groups of a 64-antenna, four-product array: 4 x 64 autocorrelations, then
4 x 2016 cross-correlations (256 + 8064 = 8320 columns). Amplitudes are Rayleigh noise with
exact ties; about 1/16 of the samples are flagged. The result of the warm-up calls is compared
with ``rfi.host.RangePercentilesHost`` on sampled rows, bit for bit.

Timed in alternation, in the same rounds:

* the operation with ``mask=0xFF``;
* the operation with ``use_flags=False``;
* eight ``Percentile5`` operations (complex, one ``column_range`` each) run back to back,
  which is what a caller had before -- without the eight OR reductions it also needs;
* the complex64 transpose of the same shape (8 bytes read and 8 written per sample), as the
  yardstick for streaming speed; the operation reads 9 (8 without flags) bytes per sample once.

Every shape is measured in a process of its own, started under a time limit; the first one
that fails ends the run.

Usage: ``python tools/time_range_percentiles.py [--rounds N] [--calls N] [--json OUT]
[--shape CxB ...]``.
"""

import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = ["4096x8320", "512x8320"]
SAMPLED_ROWS = 8
CHILD_SECONDS = 240
ANTENNAS = 64


def display_ranges(baselines):
    """Four groups of autocorrelations, then four of cross-correlations, filling the row."""
    cross = ANTENNAS * (ANTENNAS - 1) // 2
    if baselines != 4 * (ANTENNAS + cross):
        sys.exit(f"the display groups need {4 * (ANTENNAS + cross)} baselines")
    ranges = [(k * ANTENNAS, (k + 1) * ANTENNAS) for k in range(4)]
    return ranges + [(4 * ANTENNAS + k * cross, 4 * ANTENNAS + (k + 1) * cross) for k in range(4)]


def measure(channels, baselines, rounds, calls):
    """One shape, in this process."""
    import numpy as np

    from katsdpsigproc_amd import accel, percentile, transpose
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

    ranges = display_ranges(baselines)
    samples = channels * baselines
    context = accel.create_some_context(interactive=False)
    queue = context.create_command_queue()
    masked = ingest.RangePercentilesTemplate(context, mask=0xFF).instantiate(
        queue, channels, baselines, ranges)  # fmt: skip
    plain = ingest.RangePercentilesTemplate(context, use_flags=False).instantiate(
        queue, channels, baselines, ranges)  # fmt: skip
    masked.ensure_all_bound()
    plain.bind(data=masked.buffer("data"))
    plain.ensure_all_bound()
    # 512 distinct rows, repeated: noise quantised to 2^-6 for ties, 1/16 flagged
    rs = np.random.RandomState(1)
    distinct = min(channels, 512)
    block = np.rint((rs.standard_normal((distinct, baselines))
                     + 1j * rs.standard_normal((distinct, baselines))) * 64) / 64  # fmt: skip
    data = np.tile(block.astype(np.complex64), (-(-channels // distinct), 1))[:channels]
    block = np.where(rs.random_sample((distinct, baselines)) < 1 / 16, 0x10, 0).astype(np.uint8)
    flags = np.tile(block, (-(-channels // distinct), 1))[:channels]
    masked.buffer("data").set(queue, data)
    masked.buffer("flags").set(queue, flags)

    template5 = percentile.Percentile5Template(context, baselines, is_amplitude=False)
    old = [template5.instantiate(queue, (channels, baselines), r) for r in ranges]
    old[0].ensure_all_bound()
    old[0].buffer("src").set(queue, data)
    for fn in old[1:]:
        fn.bind(src=old[0].buffer("src"))
        fn.ensure_all_bound()

    def eight():
        for fn in old:
            fn()

    yardstick = transpose.TransposeTemplate(context, np.complex64, "float2").instantiate(
        queue, (channels, baselines))  # fmt: skip
    yardstick.ensure_all_bound()
    yardstick.buffer("src").set(queue, data)
    for _ in range(3):
        yardstick()
        masked()
        plain()
        eight()
    queue.finish()
    rows = np.unique(rs.randint(0, channels, SAMPLED_ROWS))
    want = host.RangePercentilesHost(ranges, 0xFF)(data[rows], flags[rows])
    for w, name in zip(want, ("percentiles", "counts", "range_flags")):
        got = np.ascontiguousarray(masked.buffer(name).get(queue)[..., rows])
        np.testing.assert_array_equal(got.view(np.uint8), np.ascontiguousarray(w).view(np.uint8))
    want = host.RangePercentilesHost(ranges)(data[rows])
    for w, name in zip(want[:2], ("percentiles", "counts")):
        got = np.ascontiguousarray(plain.buffer(name).get(queue)[..., rows])
        np.testing.assert_array_equal(got.view(np.uint8), np.ascontiguousarray(w).view(np.uint8))
    for r, fn in enumerate(old):  # (no NaN in the data: the same five rows)
        got = np.ascontiguousarray(fn.buffer("dest").get(queue)[:, rows])
        np.testing.assert_array_equal(got.view(np.uint32), np.ascontiguousarray(want[0][r]).view(np.uint32))

    timed = time_rounds(queue, [masked, plain, eight, yardstick])
    in_range = channels * sum(stop - start for start, stop in ranges)
    run = {"device": context.device.name, "channels": channels, "baselines": baselines,
           "ranges": ranges, "rounds": rounds, "calls": calls, "verified": True,
           "masked": timed[0], "no_flags": timed[1], "eight_percentile5": timed[2],
           "transpose": timed[3], "masked_bytes": int(in_range * 9),
           "no_flags_bytes": int(in_range * 8), "transpose_bytes": int(samples * 16)}  # fmt: skip
    for name in ("masked", "no_flags", "transpose"):
        run[name]["bytes_per_s"] = run[name + "_bytes"] / (run[name]["median_ms"] * 1e-3)
    run["eight_percentile5"]["bytes_per_s"] = in_range * 8 / (timed[2]["median_ms"] * 1e-3)
    run["eight_over_masked"] = timed[2]["median_ms"] / timed[0]["median_ms"]
    run["eight_over_no_flags"] = timed[2]["median_ms"] / timed[1]["median_ms"]
    run["masked_rate_over_transpose_rate"] = (run["masked"]["bytes_per_s"]
                                              / run["transpose"]["bytes_per_s"])  # fmt: skip
    run["no_flags_rate_over_transpose_rate"] = (run["no_flags"]["bytes_per_s"]
                                                / run["transpose"]["bytes_per_s"])  # fmt: skip
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
        print(f"  {shape}: mask 0xFF {text(run['masked'])}, "
              f"{run['masked']['bytes_per_s'] / 1e12:.2f} TB/s; no flags {text(run['no_flags'])}; "
              f"eight Percentile5 {text(run['eight_percentile5'])}, "
              f"{run['eight_over_masked']:.2f} x the masked one; transpose "
              f"{text(run['transpose'])}, {run['transpose']['bytes_per_s'] / 1e12:.2f} TB/s; "
              f"rate / transpose rate = {run['masked_rate_over_transpose_rate']:.2f}",
              flush=True)  # fmt: skip
        runs.append(run)
    if args.json:
        with open(args.json, "w") as f:
            json.dump({"runs": runs}, f, indent=1)


if __name__ == "__main__":
    main()
