#!/usr/bin/env python3
"""Time flag-aware averaging (``rfi.device.AccumulateTemplate`` / ``FinaliseTemplate``)
against what torch can do on the same device buffers, with the transpose kernel as the
yardstick for streaming speed in the same session.

Device time from event pairs on one stream around single calls, data resident on the device,
after a warm-up; every figure is the median of RUNS calls with the fastest and slowest beside
it. Shape 4096 x 32768 by default: the accumulators alone are 1.6 GiB, far beyond the 256 MiB
Infinity Cache, so every call streams from and to HBM. 1/16 of the samples are flagged.

* accumulate: with weights, without, and with weights and a CHANNEL mask, each in alternation
  with the torch composite a caller can write today (``where`` / ``mul`` / ``add_`` /
  ``bitwise_or_`` on tensors that wrap the operation's own buffers).
* finalise: channel_factor 1 and 8, clear on and off, and a torch composite for clear off.
* transpose: float32, same shape (reads and writes 4 bytes per sample).

The first and last 8 rows of the accumulators and of the outputs are checked against
``rfi.host.AveragerHost`` outside the timed region. Bytes are the bytes each launch must
move, computed from the shape. Usage:
``python tools/time_average.py [--channels C] [--baselines B] [--runs N] [--json OUT]``.
"""

import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402  (before the native library: one HIP runtime per process)

from katsdpsigproc_amd import accel, hip, transpose  # noqa: E402
from katsdpsigproc_amd.rfi import device, host  # noqa: E402

HBM_COPY_RATE = 6.3e12  # bytes/s, achievable
EDGE = 8  # rows checked at either end
ACC = ("acc_vis", "acc_weights", "acc_flags")
OUT = ("vis", "weights", "flags")


class _View:
    """A device buffer under another element type, for ``torch.as_tensor``."""

    def __init__(self, buffer, shape, typestr):
        self.__cuda_array_interface__ = {"shape": tuple(shape), "typestr": typestr,
                                         "data": (buffer.ptr, False), "version": 2}  # fmt: skip


def as_torch(array):
    """Tensor over the data of a 1-D or 2-D DeviceArray (padding sliced off); complex64 comes
    as float32 with a last axis of 2."""
    shape, padded = array.shape, array.padded_shape
    if array.dtype == np.complex64:
        t = torch.as_tensor(_View(array.buffer, padded + (2,), "<f4"), device="cuda")
    else:
        t = torch.as_tensor(_View(array.buffer, padded, array.dtype.str), device="cuda")
    assert t.data_ptr() == array.buffer.ptr
    return t[: shape[0], : shape[1]] if len(shape) == 2 else t[: shape[0]]


def timed(queue, functions, runs, before=None):
    """Milliseconds of each function: `runs` single calls between event pairs, the functions
    taking turns; `before` (untimed) runs ahead of every call."""
    times = [[] for _ in functions]
    for _ in range(runs):
        for i, fn in enumerate(functions):
            if before is not None:
                before()
            start = queue.enqueue_marker()
            fn()
            stop = queue.enqueue_marker()
            times[i].append(stop.time_since(start) * 1e3)
    return [{"median_ms": float(np.median(t)), "min_ms": min(t), "max_ms": max(t)} for t in times]


def rate(entry, n_bytes):
    entry["bytes"] = int(n_bytes)
    entry["bytes_per_s"] = n_bytes / (entry["median_ms"] * 1e-3)
    entry["share_of_hbm_copy_rate"] = entry["bytes_per_s"] / HBM_COPY_RATE
    return entry


def show(label, entry, other=None):
    text = (f"  {label}: {entry['median_ms']:.3f} ms ({entry['min_ms']:.3f}..{entry['max_ms']:.3f}), "
            f"{entry['bytes'] / 1e9:.2f} GB, {entry['bytes_per_s'] / 1e12:.2f} TB/s")  # fmt: skip
    if other is not None:
        text += (f"; torch {other['median_ms']:.3f} ms "
                 f"({other['min_ms']:.3f}..{other['max_ms']:.3f})")  # fmt: skip
    print(text, flush=True)


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


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--channels", type=int, default=4096)
    parser.add_argument("--baselines", type=int, default=32768)
    parser.add_argument("--runs", type=int, default=20)
    parser.add_argument("--json")
    args = parser.parse_args()
    channels, baselines, runs = args.channels, args.baselines, args.runs
    samples = channels * baselines
    context = accel.create_some_context(interactive=False)
    # torch's current stream, so that one pair of events brackets either contender
    queue = hip.CommandQueue(context, stream=torch.cuda.current_stream().cuda_stream)
    result = {"device": context.device.name, "channels": channels, "baselines": baselines,
              "runs": runs, "density": 1.0 / 16.0, "accumulate": [], "finalise": []}  # fmt: skip
    gen = torch.Generator(device="cuda").manual_seed(1)

    # ---------------------------------------------------------------- accumulate
    for use_weights, mode in ((True, "NONE"), (False, "NONE"), (True, "CHANNEL")):
        flags_mode = device.BackgroundFlags[mode]
        op = device.AccumulateTemplate(context, use_weights, flags_mode).instantiate(
            queue, channels, baselines)  # fmt: skip
        op.ensure_all_bound()
        t = {name: as_torch(op.buffer(name)) for name in op.slots}
        t["vis"].copy_(torch.randn(t["vis"].shape, generator=gen, device="cuda"))
        hit = torch.rand(t["flags"].shape, generator=gen, device="cuda") < 1.0 / 16.0
        t["flags"].copy_(torch.randint(1, 256, t["flags"].shape, generator=gen, device="cuda",
                                       dtype=torch.uint8) * hit)  # fmt: skip
        del hit
        if use_weights:
            t["weights"].copy_(torch.rand(t["weights"].shape, generator=gen, device="cuda") * 1.5 + 0.5)
        if flags_mode:
            t["input_flags"].copy_((torch.rand(channels, generator=gen, device="cuda") < 1.0 / 16.0)
                                   .to(torch.uint8) * 0x40)  # fmt: skip

        def clear_acc(op=op):
            for name in ACC:
                op.buffer(name).zero(queue)

        def torch_accumulate(t=t, use_weights=use_weights, flags_mode=flags_mode):
            f = t["flags"] | t["input_flags"][:, None] if flags_mode else t["flags"]
            bad = f != 0
            if use_weights:
                we = torch.where(bad, t["weights"] * 2.0**-64, t["weights"])
            else:
                we = torch.where(bad, 2.0**-64, 1.0)
            t["acc_vis"].add_(we[..., None] * t["vis"])
            t["acc_weights"].add_(we)
            t["acc_flags"].bitwise_or_(f)

        # two dumps from zero, checked at the edges; also the warm-up
        clear_acc()
        op()
        op()
        reference = host.AveragerHost(2 * EDGE, baselines, 1, flags_mode)
        weights = edge_rows(t["weights"]) if use_weights else None
        mask = {"input_flags": edge_rows(t["input_flags"])} if flags_mode else {}
        for _ in range(2):
            reference.add(edge_rows(t["vis"]), edge_rows(t["flags"]), weights, **mask)
        want = (reference.acc_vis, reference.acc_weights, reference.acc_flags)
        for name, w in zip(ACC, want):
            same(w, edge_rows(t[name]), f"{name} after the operation")
        clear_acc()
        torch_accumulate()
        torch_accumulate()
        torch_matches = True
        for name, w in zip(ACC, want):
            try:
                same(w, edge_rows(t[name]), f"{name} after the torch composite")
            except AssertionError as exc:  # a contender, not the code under test
                print("  note:", exc, flush=True)
                torch_matches = False
        queue.finish()
        op_ms, torch_ms = timed(queue, [op, torch_accumulate], runs)
        n_bytes = samples * (8 + 1 + (4 if use_weights else 0) + 2 * (8 + 4 + 1))
        n_bytes += channels if flags_mode else 0
        run = {"use_weights": use_weights, "input_flags": mode, "verified": True,
               "op": rate(op_ms, n_bytes), "torch": torch_ms,
               "torch_matches": torch_matches, "op_faster": op_ms["median_ms"] < torch_ms["median_ms"]}  # fmt: skip
        show(f"accumulate weights={use_weights!s:5} input_flags={mode:7}", op_ms, torch_ms)
        result["accumulate"].append(run)
        del t, op, reference
        torch.cuda.empty_cache()

    # ------------------------------------------------------------------ finalise
    for channel_factor in (1, 8):
        ops = {clear: device.FinaliseTemplate(context, channel_factor, clear).instantiate(
            queue, channels, baselines) for clear in (False, True)}  # fmt: skip
        seq = accel.OperationSequence(
            queue, [("keep", ops[False]), ("clear", ops[True])],
            compounds={name: ["keep:" + name, "clear:" + name] for name in ACC + OUT})
        seq.ensure_all_bound()
        t = {name: as_torch(seq.buffer(name)) for name in ACC + OUT}
        saved = {}

        def fill(t=t, saved=saved):
            """Accumulators as two dumps would leave them (1/16 of them flagged in both)."""
            if not saved:
                bad = torch.rand(t["acc_flags"].shape, generator=gen, device="cuda") < 1.0 / 16.0
                w = (torch.rand(t["acc_weights"].shape, generator=gen, device="cuda") + 1.0)
                w = torch.where(bad, w * 2.0**-64, w)
                t["acc_weights"].copy_(w)
                t["acc_vis"].copy_(torch.randn(t["acc_vis"].shape, generator=gen, device="cuda")
                                   * w[..., None])  # fmt: skip
                t["acc_flags"].copy_(bad.to(torch.uint8) * 3)
                saved.update({name: t[name].clone() for name in ACC})
            else:
                for name in ACC:
                    t[name].copy_(saved[name])

        def torch_finalise(t=t, cf=channel_factor):
            rows = channels // cf
            w = t["acc_weights"].view(rows, cf, baselines).sum(1)
            v = t["acc_vis"].view(rows, cf, baselines, 2).sum(1)
            # (the accumulated flags here are 0 or 3, for which the maximum is the OR)
            fl = t["acc_flags"].view(rows, cf, baselines).amax(1)
            allbad = w < 2.0**-32
            w = torch.where(allbad, w * 2.0**64, w)
            v = torch.where(allbad[..., None], v * 2.0**64, v)
            t["vis"].copy_(torch.where((w > 0)[..., None], v / w[..., None], 0.0))
            t["weights"].copy_(w)
            t["flags"].copy_(torch.where(allbad, fl, 0))

        fill()
        reference = host.AveragerHost(2 * EDGE * channel_factor, baselines, channel_factor)
        take = EDGE * channel_factor
        for name, dest in zip(ACC, (reference.acc_vis, reference.acc_weights, reference.acc_flags)):
            a = torch.cat([t[name][:take], t[name][-take:]]).cpu().numpy()
            dest[...] = a.view(np.complex64)[..., 0] if a.ndim == 3 else a
        want = reference.finalise()
        for clear in (False, True):
            ops[clear]()
            for name, w in zip(OUT, want):
                same(w, edge_rows(t[name]), f"{name}, channel_factor {channel_factor}, clear {clear}")
        for name in ACC:
            if bool(t[name].any()):
                raise AssertionError(f"{name} was not cleared")
        queue.finish()
        in_bytes = samples * 13
        out_bytes = samples // channel_factor * 13
        fill()
        keep_ms, torch_ms = timed(queue, [ops[False], torch_finalise], runs)
        (clear_ms,) = timed(queue, [ops[True]], runs, before=fill)
        run = {"channel_factor": channel_factor, "verified": True,
               "op": rate(keep_ms, in_bytes + out_bytes), "torch": torch_ms,
               "op_clear": rate(clear_ms, 2 * in_bytes + out_bytes)}  # fmt: skip
        show(f"finalise channel_factor={channel_factor} clear=False", keep_ms, torch_ms)
        show(f"finalise channel_factor={channel_factor} clear=True ", clear_ms)
        result["finalise"].append(run)
        del t, saved, seq, ops, reference
        torch.cuda.empty_cache()

    # ----------------------------------------------------------------- transpose
    op = transpose.TransposeTemplate(context, np.float32, "float").instantiate(
        queue, (channels, baselines))  # fmt: skip
    op.ensure_all_bound()
    as_torch(op.buffer("src")).copy_(torch.randn(channels, baselines, generator=gen, device="cuda"))
    for _ in range(3):
        op()
    queue.finish()
    (transpose_ms,) = timed(queue, [op], runs)
    result["transpose"] = rate(transpose_ms, samples * 8)
    show("transpose float32", transpose_ms)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
