#!/usr/bin/env python3
"""Time the per-input delay fit (``rfi.ingest.FitDelaysTemplate``) against what it replaces or
resembles.

Device time from events on one stream, data resident on the device, after a warm-up; every
figure is the median over ROUNDS rounds of CALLS calls, with the fastest and slowest round
beside it as the run-to-run spread. Shapes: 4096 channels x 128 inputs with a transform of 16384
and 1024 x 128 with 4096, noisy tones with a tenth of the channels missing, with ``status`` and
``model``, ``refine`` 0 and 3, and ``refine`` 3 without ``model`` (what the strided stores of the
model cost). The result of the warm-up call is compared with ``rfi.host.FitDelaysHost``, every
output bit for bit (a NaN for a NaN).

Timed in alternation with the operation, in the same rounds: the ``Fft`` operation (hipFFT) on
a batch of n_inputs contiguous complex64 transforms of n_fft, which is the transform alone, of
rows that are already transposed and padded, without the peak, the refinement or the model; and
the round trip the operation removes, ``gains`` copied to the host and a ``model`` copied back
(wall-clock time of the two blocking copies, pageable host memory, without the host's fit).

Every shape is measured in a process of its own, started under a time limit; the first one
that fails ends the run.

Usage: ``python tools/time_fit_delays.py [--rounds N] [--calls N] [--json OUT]
[--shape CHANNELSxINPUTSxNFFT ...]``.
"""

import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = ["4096x128x16384", "1024x128x4096"]
#: (refine, model)
VARIANTS = [(0, True), (3, True), (3, False)]
CHILD_SECONDS = 300


def measure(channels, n_inputs, n_fft, rounds, calls):
    """One shape, every refine, in this process."""
    import numpy as np

    from katsdpsigproc_amd import accel, fft
    from katsdpsigproc_amd.rfi import host, ingest

    def summary(t):
        return {"median_ms": float(np.median(t)), "min_ms": min(t), "max_ms": max(t)}

    def same(want, got, what):
        want, got = np.ascontiguousarray(want), np.ascontiguousarray(got)
        if want.dtype == np.uint8:
            assert np.array_equal(want, got), what
            return
        part, word = (np.float64, np.uint64) if want.dtype == np.float64 else (np.float32, np.uint32)
        nan = np.isnan(want.view(part))
        equal = want.view(word) == got.view(word)
        assert np.all(np.where(nan, np.isnan(got.view(part)), equal)), what

    context = accel.create_some_context(interactive=False)
    queue = context.create_command_queue()
    rs = np.random.RandomState(1)
    c = np.arange(channels)[:, np.newaxis]
    shape = (channels, n_inputs)
    gains = np.exp(2j * np.pi * (c * rs.uniform(-0.5, 0.5, n_inputs) + rs.random_sample(n_inputs)))
    gains *= 1 + 0.3 * rs.standard_normal(shape)
    gains += 0.3 * np.sqrt(0.5) * (rs.standard_normal(shape) + 1j * rs.standard_normal(shape))
    gains = gains.astype(np.complex64)
    status = (rs.random_sample(channels) < 0.1).astype(np.uint8)
    gains[status != 0] = complex(np.nan, np.nan)

    batch = (n_inputs, n_fft)
    yardstick = fft.FftTemplate(context, 1, batch, np.complex64, np.complex64, batch,
                                batch).instantiate(queue, fft.FftMode.FORWARD)  # fmt: skip
    yardstick.ensure_all_bound()
    padded = np.zeros(batch, np.complex64)
    padded[:, :channels] = np.where(np.isnan(gains.real), 0, gains).T
    yardstick.buffer("src").set(queue, padded)

    runs = []
    for refine, with_model in VARIANTS:
        op = ingest.FitDelaysTemplate(context, 1e6, n_fft, refine, model=with_model).instantiate(
            queue, channels, n_inputs)  # fmt: skip
        op.ensure_all_bound()
        op.buffer("gains").set(queue, gains)
        op.buffer("status").set(queue, status)
        op()
        queue.finish()
        want = host.FitDelaysHost(1e6, n_fft, refine)(gains, status)
        names = ("delays", "phasors", "amplitudes", "fit_status", "model")
        for name, w in zip(names, want):
            if name in op.slots:
                same(w, op.buffer(name).get(queue), name)
        for _ in range(2):
            yardstick()
            op()
        queue.finish()
        model = accel.DeviceArray(context, shape, np.complex64)
        times = {"op": [], "fft": [], "round_trip": []}
        for _ in range(rounds):
            for name, fn in (("op", op), ("fft", yardstick)):
                start = queue.enqueue_marker()
                for _ in range(calls):
                    fn()
                stop = queue.enqueue_marker()
                times[name].append(stop.time_since(start) / calls * 1e3)
            queue.finish()
            begin = time.perf_counter()
            for _ in range(calls):
                op.buffer("gains").get(queue)
                model.set(queue, want[4])
            queue.finish()
            times["round_trip"].append((time.perf_counter() - begin) / calls * 1e3)
        run = {"refine": refine, "model": with_model, "fitted": int(np.count_nonzero(want[3] == 0))}
        run.update({name: summary(t) for name, t in times.items()})
        runs.append(run)
        del op
    return {"device": context.device.name, "channels": channels, "n_inputs": n_inputs,
            "n_fft": n_fft, "rounds": rounds, "calls": calls, "verified": True,
            "runs": runs}  # fmt: skip


def text(entry):
    return f"{entry['median_ms']:.4f} ms ({entry['min_ms']:.4f}..{entry['max_ms']:.4f})"


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--shape", action="append", help="CHANNELSxINPUTSxNFFT (repeatable)")
    parser.add_argument("--rounds", type=int, default=7)
    parser.add_argument("--calls", type=int, default=20)
    parser.add_argument("--json")
    parser.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    args = parser.parse_args()
    shapes = args.shape or SHAPES
    if args.child:
        channels, n_inputs, n_fft = (int(n) for n in shapes[0].split("x"))
        print(json.dumps(measure(channels, n_inputs, n_fft, args.rounds, args.calls)))
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
        for run in result["runs"]:
            variant = f"refine {run['refine']}{'' if run['model'] else ', no model'}"
            print(f"  {variant}: op {text(run['op'])}; Fft of {result['n_inputs']} x "
                  f"{result['n_fft']} {text(run['fft'])}; gains to the host and a model back "
                  f"{text(run['round_trip'])}; {run['fitted']} of {result['n_inputs']} fitted",
                  flush=True)  # fmt: skip
        results.append(result)
    if args.json:
        with open(args.json, "w") as f:
            json.dump({"runs": results}, f, indent=1)


if __name__ == "__main__":
    main()
