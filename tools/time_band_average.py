#!/usr/bin/env python3
"""Time the band averages (``rfi.ingest.BandAverageTemplate``) against the two ``MaskedSum``
launches they replace, and against a streaming kernel.

Device time from events on one stream, data resident on the device, after a warm-up; every
figure is the median over ROUNDS rounds (at least 10) of CALLS calls, with the fastest and
slowest round beside it as the run-to-run spread. Shapes: 4096 x 8320 complex64 (272 MB: from
HBM every call) and 512 x 8320 (what ``channel_factor=8`` leaves of it, which fits the
Infinity Cache). Data is normal noise, about 1/16 of the samples are flagged, and the series
are sub-bands of random positive weights that together cover the band. The result of the
warm-up calls is compared with ``rfi.host.BandAverageHost`` on sampled baselines, bit for bit.

Timed in alternation, in the same rounds:

* the operation with one series and ``mask=0xFF``;
* the operation with eight series and ``mask=0xFF``;
* the operation with one series and ``use_flags=False``;
* two ``MaskedSum`` launches on the same buffer, complex and ``use_amplitudes``, which is what
  a caller has today for ONE series (every flagged and NaN sample included, no weight sum);
* the float32 transpose of (channels * 9 / 8) x baselines: 4 bytes read and 4 written per
  element, the byte count of the 9 bytes per sample that the operation reads, as the yardstick
  for streaming speed.

Every shape is measured in a process of its own, started under a time limit; the first one
that fails ends the run.

Usage: ``python tools/time_band_average.py [--rounds N] [--calls N] [--json OUT]
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
SAMPLED_BASELINES = 16
CHILD_SECONDS = 240
NAMES = ("mean", "mean_amplitude", "weight_sums", "counts", "series_flags")


def measure(channels, baselines, rounds, calls):
    """One shape, in this process."""
    import numpy as np

    from katsdpsigproc_amd import accel, maskedsum, transpose
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

    samples = channels * baselines
    context = accel.create_some_context(interactive=False)
    queue = context.create_command_queue()
    one = ingest.BandAverageTemplate(context, mask=0xFF).instantiate(queue, channels, baselines, 1)
    eight = ingest.BandAverageTemplate(context, mask=0xFF).instantiate(queue, channels, baselines, 8)
    plain = ingest.BandAverageTemplate(context, use_flags=False).instantiate(
        queue, channels, baselines, 1)  # fmt: skip
    one.ensure_all_bound()
    for fn in (eight, plain):
        fn.bind(data=one.buffer("data"))
    eight.bind(flags=one.buffer("flags"))
    eight.ensure_all_bound()
    plain.ensure_all_bound()
    # 512 distinct rows, repeated; 1/16 flagged
    rs = np.random.RandomState(1)
    distinct = min(channels, 512)
    block = rs.standard_normal((distinct, baselines)) + 1j * rs.standard_normal((distinct, baselines))
    data = np.tile(block.astype(np.complex64), (-(-channels // distinct), 1))[:channels]
    block = np.where(rs.random_sample((distinct, baselines)) < 1 / 16, 0x10, 0).astype(np.uint8)
    flags = np.tile(block, (-(-channels // distinct), 1))[:channels]
    weights8 = np.zeros((8, channels), np.float32)
    for k in range(8):  # eight sub-bands that together cover the band
        part = slice(k * channels // 8, (k + 1) * channels // 8)
        weights8[k, part] = 0.5 + rs.random_sample(part.stop - part.start)
    weights1 = (0.5 + rs.random_sample((1, channels))).astype(np.float32)
    weights1[0, : channels // 16] = 0  # the band's edge is left out
    one.buffer("data").set(queue, data)
    one.buffer("flags").set(queue, flags)
    one.buffer("channel_weights").set(queue, weights1)
    plain.buffer("channel_weights").set(queue, weights1)
    eight.buffer("channel_weights").set(queue, weights8)

    sums = [maskedsum.MaskedSumTemplate(context, use_amplitudes).instantiate(
        queue, (channels, baselines)) for use_amplitudes in (False, True)]  # fmt: skip
    for fn in sums:
        fn.bind(src=one.buffer("data"))
        fn.ensure_all_bound()
        fn.buffer("mask").set(queue, weights1[0])

    def two_sums():
        for fn in sums:
            fn()

    yardstick = transpose.TransposeTemplate(context, np.float32, "float").instantiate(
        queue, (channels * 9 // 8, baselines))  # fmt: skip
    yardstick.ensure_all_bound()
    yardstick.buffer("src").zero(queue)

    functions = [one, eight, plain, two_sums, yardstick]
    for _ in range(3):
        for fn in functions:
            fn()
    queue.finish()
    cols = np.unique(rs.randint(0, baselines, SAMPLED_BASELINES))
    sampled, sampled_flags = np.ascontiguousarray(data[:, cols]), np.ascontiguousarray(flags[:, cols])
    for fn, weights, want in (
            (one, weights1, host.BandAverageHost(0xFF)(sampled, weights1, sampled_flags)),
            (eight, weights8, host.BandAverageHost(0xFF)(sampled, weights8, sampled_flags)),
            (plain, weights1, host.BandAverageHost()(sampled, weights1))):  # fmt: skip
        for w, name in zip(want, NAMES):
            if w is not None:
                got = np.ascontiguousarray(fn.buffer(name).get(queue)[:, cols])
                np.testing.assert_array_equal(got.view(np.uint8), np.ascontiguousarray(w).view(np.uint8))
    # the two sums give the numerators of `plain` to the tolerance of their own test
    want = host.BandAverageHost()(sampled, weights1)
    np.testing.assert_allclose(sums[0].buffer("dest").get(queue)[cols], want[0][0] * want[2][0],
                               rtol=1e-4, atol=1e-2 * np.sqrt(channels))  # fmt: skip

    timed = time_rounds(queue, functions)
    keys = ("one_series", "eight_series", "one_series_no_flags", "two_maskedsums", "transpose")
    n_blocks = -(-channels // host.BandAverageHost.BLOCK)
    partials = 2 * 20 * n_blocks * baselines  # written and read back, per series
    out_bytes = {"one_series": 21 * baselines, "eight_series": 8 * 21 * baselines,
                 "one_series_no_flags": 20 * baselines}  # fmt: skip
    run = {"device": context.device.name, "channels": channels, "baselines": baselines,
           "rounds": rounds, "calls": calls, "verified": True}  # fmt: skip
    run.update(dict(zip(keys, timed)))
    run["one_series"]["bytes"] = samples * 9 + partials + channels * 4 + out_bytes["one_series"]
    run["eight_series"]["bytes"] = (samples * 9 + 8 * partials + 8 * channels * 4
                                    + out_bytes["eight_series"])  # fmt: skip
    run["one_series_no_flags"]["bytes"] = (samples * 8 + partials + channels * 4
                                           + out_bytes["one_series_no_flags"])  # fmt: skip
    run["two_maskedsums"]["bytes"] = samples * 16 + 2 * channels * 4 + 12 * baselines
    run["transpose"]["bytes"] = (channels * 9 // 8) * baselines * 8
    for key in keys:
        run[key]["bytes_per_s"] = run[key]["bytes"] / (run[key]["median_ms"] * 1e-3)
    run["two_maskedsums_over_one_series"] = timed[3]["median_ms"] / timed[0]["median_ms"]
    run["eight_series_over_one_series"] = timed[1]["median_ms"] / timed[0]["median_ms"]
    run["one_series_over_transpose"] = timed[0]["median_ms"] / timed[4]["median_ms"]
    return run


def text(entry):
    return (f"{entry['median_ms']:.3f} ms ({entry['min_ms']:.3f}..{entry['max_ms']:.3f}), "
            f"{entry['bytes_per_s'] / 1e12:.2f} TB/s")  # fmt: skip


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--shape", action="append", help="CHANNELSxBASELINES (repeatable)")
    parser.add_argument("--rounds", type=int, default=10)
    parser.add_argument("--calls", type=int, default=10)
    parser.add_argument("--json")
    parser.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    args = parser.parse_args()
    if args.rounds < 10:
        sys.exit("the median is taken over at least 10 rounds")
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
        print(f"  {shape}: one series {text(run['one_series'])}; eight series "
              f"{text(run['eight_series'])}; one series, no flags "
              f"{text(run['one_series_no_flags'])}; two MaskedSum {text(run['two_maskedsums'])}, "
              f"{run['two_maskedsums_over_one_series']:.2f} x one series; float32 transpose "
              f"{text(run['transpose'])}", flush=True)  # fmt: skip
        runs.append(run)
    if args.json:
        with open(args.json, "w") as f:
            json.dump({"runs": runs}, f, indent=1)


if __name__ == "__main__":
    main()
