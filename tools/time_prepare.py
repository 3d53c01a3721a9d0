#!/usr/bin/env python3
"""Time the preparation of a correlator dump (``rfi.ingest.PrepareTemplate``) against what a
caller could do without it, and against a streaming kernel of similar traffic.

Device time from events on one stream, data resident on the device, after a warm-up; every
figure is the median over ROUNDS rounds of CALLS calls, with the fastest and slowest round
beside it as the run-to-run spread. Shape 4096 x 32768 from 32768 input baselines (a dump of
1 GiB: from HBM every call), with and without weights, for three index maps:

* ``identity``: output baseline j is input baseline j;
* ``random``: a random permutation;
* ``meerkat``: the input holds the four polarisation products of an antenna pair next to each
  other (128 antennas, the autocorrelations first, 8192 pairs), the output is sorted by
  product first: ``source[q * 8192 + p] = 4 p + q``.

``auto_source`` is, for every map, the pair of HH / VV autocorrelations that belongs to the
input baseline: 256 distinct addresses per row. The dump is integer noise of 1e5 with
autocorrelations around 1e6 and 1 % lost samples. The result of the warm-up call is checked
against ``rfi.host.PrepareHost`` on sampled rows.

Timed in alternation with the operation, in the same rounds:

* the torch composite a caller can write today on tensors that wrap the operation's own
  buffers: ``index_select``, two casts, a multiply, a compare and the masked fills, and for
  the weights two more gathers, the products and a division (its ``vis`` and ``input_flags``
  are checked exactly, its weights to 1e-6: torch's division is not correctly rounded);
* ``rfi.device.Accumulate`` without weights on the operation's ``vis`` and ``input_flags``:
  35 bytes per sample, all of them streamed, against the 17 (21 with weights) of this
  operation, 8 of which are gathered.

And, on the same buffers, the instance with flags per baseline (two classes of static mask,
the second for the first eighth of the baselines only, the last quarter with none, and
``baseline_flags`` set on 3 % of the baselines; ``ksp_prepare_flags``) against

* the option-free instance above: the cost of the feature;
* what a caller does without it: the option-free instance followed by the torch composite
  ``input_flags |= baseline_flags[None, :] | masks[index]`` (one gather, two ORs and a pass
  over ``input_flags``; "no mask" is a row of zeros behind the classes).

Both are checked bit for bit against ``rfi.host.PrepareHost`` on the sampled rows.

Usage: ``python tools/time_prepare.py [--channels C] [--baselines B] [--rounds N] [--calls N]
[--json OUT]`` (`baselines` a multiple of 4, at least 1024).
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

LOST = -(2**31)
SCALE, LOST_FLAG, WEIGHT_SCALE = 2.0**-8, 8, 2.0**24
ANTENNAS = 128
SAMPLED_ROWS = 8
CLASSES, MASK_BITS, OFF_TARGET = 2, (0x20, 0x10), 0x40


class _View:
    """A device buffer under another element type or shape, for ``torch.as_tensor``."""

    def __init__(self, buffer, shape, typestr):
        self.__cuda_array_interface__ = {"shape": tuple(shape), "typestr": typestr,
                                         "data": (buffer.ptr, False), "version": 2}  # fmt: skip


def as_torch(array):
    """Tensor over the data of a DeviceArray (row padding sliced off); complex64 comes as
    float32 with a last axis of 2."""
    shape, padded = array.shape, array.padded_shape
    if array.dtype == np.complex64:
        t = torch.as_tensor(_View(array.buffer, padded + (2,), "<f4"), device="cuda")
    else:
        t = torch.as_tensor(_View(array.buffer, padded, array.dtype.str), device="cuda")
    assert t.data_ptr() == array.buffer.ptr
    return t[:, : shape[1]] if len(shape) >= 2 else t


def index_maps(baselines):
    """{name: (source, auto_source)} for `baselines` = 4 x pairs input and output baselines."""
    pairs = baselines // 4
    # input baseline 4 p + q: product q (HH, HV, VH, VV) of pair p; pairs: the autocorrelations
    # of the antennas first, then the cross-correlations row by row, as many as fit
    ant = [(a, a) for a in range(ANTENNAS)]
    ant += [(a, b) for a in range(ANTENNAS) for b in range(a + 1, ANTENNAS)]
    ant = np.array(ant[:pairs])
    assert len(ant) == pairs >= ANTENNAS
    pol_a, pol_b = np.array([0, 0, 3, 3]), np.array([0, 3, 0, 3])  # HH or VV of each input
    auto_of_input = np.empty((baselines, 2), np.int32)
    for q in range(4):
        auto_of_input[q::4, 0] = 4 * ant[:, 0] + pol_a[q]
        auto_of_input[q::4, 1] = 4 * ant[:, 1] + pol_b[q]
    j = np.arange(baselines)
    sources = {
        "identity": j,
        "random": np.random.RandomState(2).permutation(baselines),
        "meerkat": 4 * (j % pairs) + j // pairs,
    }
    return {name: (s.astype(np.int32), auto_of_input[s]) for name, s in sources.items()}


def fill_dump(vis_in, gen):
    """Integer noise of 1e5, autocorrelations (HH and VV of the first ANTENNAS pairs) around
    1e6 with no imaginary part, 1 % of the other samples lost; row block by row block."""
    channels = vis_in.shape[0]
    for r0 in range(0, channels, 256):
        part = vis_in[r0 : r0 + 256]
        noise = torch.randn(part.shape, generator=gen, device="cuda") * 1e5
        part.copy_(noise.round().to(torch.int32))
        lost = torch.rand(part.shape[:2], generator=gen, device="cuda") < 0.01
        part[..., 0].masked_fill_(lost, LOST)
        autos = part[:, : 4 * ANTENNAS].view(part.shape[0], ANTENNAS, 4, 2)
        level = torch.randn(autos[:, :, ::3, 0].shape, generator=gen, device="cuda") * 1e5 + 1e6
        autos[:, :, ::3, 0] = level.round().to(torch.int32)
        autos[:, :, ::3, 1] = 0


def time_rounds(queue, functions, rounds, calls):
    """Milliseconds per call of each function: rounds x calls, the functions taking turns."""
    times = [[] for _ in functions]
    for _ in range(rounds):
        for i, fn in enumerate(functions):
            start = queue.enqueue_marker()
            for _ in range(calls):
                fn()
            stop = queue.enqueue_marker()
            times[i].append(stop.time_since(start) / calls * 1e3)
    return [{"median_ms": float(np.median(t)), "min_ms": min(t), "max_ms": max(t)} for t in times]


def torch_prepare(t, source, auto_source, use_weights):
    """The composite a caller can write with torch alone, into the operation's own outputs."""
    picked = t["vis_in"].index_select(1, source)
    lost = picked[..., 0] == LOST
    vis = picked.to(torch.float32) * SCALE
    vis.masked_fill_(lost.unsqueeze(-1), 0.0)
    t["vis"].copy_(vis)
    t["input_flags"].copy_(lost.to(torch.uint8) * LOST_FLAG)
    if use_weights:
        re = t["vis_in"][..., 0]
        power = []
        for k in (0, 1):
            p = re.index_select(1, auto_source[:, k])
            power.append(torch.where(p == LOST, 0.0, p.to(torch.float32) * SCALE))
        d = power[0] * power[1]
        some = (power[0] > 0) & (power[1] > 0) & (d > 0)
        t["weights"].copy_(torch.where(some, WEIGHT_SCALE / d, 0.0))


def flag_inputs(channels, baselines):
    """(masks, mask_index, baseline_flags) of the instance with flags per baseline."""
    rs = np.random.RandomState(4)
    masks = np.zeros((CLASSES, channels), np.uint8)
    for k, bit in enumerate(MASK_BITS):
        masks[k, rs.random_sample(channels) < 0.125] = bit
    mask_index = np.zeros(baselines, np.uint8)
    mask_index[: baselines // 8] = 1
    mask_index[-(baselines // 4) :] = 255
    baseline_flags = np.where(rs.random_sample(baselines) < 0.03, OFF_TARGET, 0).astype(np.uint8)
    return masks, mask_index, baseline_flags


def torch_flags(t, masks_t, index, baseline_flags):
    """What a caller ORs into `input_flags` after the option-free operation. `masks_t` is
    channels x (classes + 1), the last column zeros; `index` is clipped to it."""
    static = masks_t.index_select(1, index)
    t["input_flags"].bitwise_or_(static | baseline_flags.unsqueeze(0))


def text(entry):
    return f"{entry['median_ms']:.3f} ms ({entry['min_ms']:.3f}..{entry['max_ms']:.3f})"


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--channels", type=int, default=4096)
    parser.add_argument("--baselines", type=int, default=32768)
    parser.add_argument("--rounds", type=int, default=5)
    parser.add_argument("--calls", type=int, default=10)
    parser.add_argument("--json")
    args = parser.parse_args()
    channels, baselines = args.channels, args.baselines
    if baselines % 4 or baselines < 8 * ANTENNAS:
        parser.error("baselines must be a multiple of 4 and at least 1024")
    samples = channels * baselines
    context = accel.create_some_context(interactive=False)
    # torch's current stream, so that one pair of events brackets any contender
    queue = hip.CommandQueue(context, stream=torch.cuda.current_stream().cuda_stream)
    reference = host.PrepareHost(SCALE, LOST_FLAG, WEIGHT_SCALE)
    maps = index_maps(baselines)
    rows = np.unique(np.random.RandomState(3).randint(0, channels, SAMPLED_ROWS))
    result = {"device": context.device.name, "channels": channels, "baselines": baselines,
              "in_baselines": baselines, "rounds": args.rounds, "calls": args.calls,
              "runs": []}  # fmt: skip
    gen = torch.Generator(device="cuda").manual_seed(1)
    vis_in_host = None
    for use_weights in (False, True):
        op = ingest.PrepareTemplate(context, SCALE, LOST_FLAG, False, use_weights,
                                    WEIGHT_SCALE).instantiate(queue, channels, baselines)  # fmt: skip
        op.ensure_all_bound()
        op_flags = ingest.PrepareTemplate(
            context, SCALE, LOST_FLAG, True, use_weights, WEIGHT_SCALE, mask_classes=CLASSES,
            baseline_flags=True).instantiate(queue, channels, baselines)  # fmt: skip
        op_flags.bind(**{name: op.buffer(name) for name in op.slots})
        op_flags.ensure_all_bound()
        masks, mask_index, baseline_flags = flag_inputs(channels, baselines)
        op_flags.buffer("channel_flags").set(queue, masks)
        op_flags.buffer("mask_index").set(queue, mask_index)
        op_flags.buffer("baseline_flags").set(queue, baseline_flags)
        masks_t = torch.as_tensor(np.vstack([masks, np.zeros_like(masks[:1])]).T.copy(), device="cuda")
        d_index = torch.as_tensor(np.minimum(mask_index, CLASSES).astype(np.int64), device="cuda")
        d_baseline_flags = torch.as_tensor(baseline_flags, device="cuda")
        yardstick = device.AccumulateTemplate(context, use_weights=False).instantiate(
            queue, channels, baselines)  # fmt: skip
        yardstick.bind(vis=op.buffer("vis"), flags=op.buffer("input_flags"))
        yardstick.ensure_all_bound()
        for name in ("acc_vis", "acc_weights", "acc_flags"):
            yardstick.buffer(name).zero(queue)
        t = {name: as_torch(op.buffer(name)) for name in op.slots}
        fill_dump(t["vis_in"], gen)
        torch.cuda.synchronize()
        vis_in_host = t["vis_in"][torch.as_tensor(rows, device="cuda")].cpu().numpy()
        n_bytes = samples * (8 + 8 + 1 + (4 if use_weights else 0))
        for name, (source, auto_source) in maps.items():
            op.buffer("source").set(queue, source)
            if use_weights:
                op.buffer("auto_source").set(queue, auto_source)
            want = reference(vis_in_host, source, None, auto_source if use_weights else None)
            want_flags = reference(vis_in_host, source, masks[:, rows],
                                   auto_source if use_weights else None, baseline_flags, mask_index)  # fmt: skip
            d_source = torch.as_tensor(source.astype(np.int64), device="cuda")
            d_auto = torch.as_tensor(auto_source.astype(np.int64), device="cuda")
            outputs = ["vis", "input_flags"] + (["weights"] if use_weights else [])

            def sampled(which):
                got = t[which][torch.as_tensor(rows, device="cuda")].cpu().numpy()
                return got.view(np.complex64)[..., 0] if which == "vis" else got

            def composite():
                torch_prepare(t, d_source, d_auto, use_weights)

            def today():
                op()
                torch_flags(t, masks_t, d_index, d_baseline_flags)

            def check(expected):
                queue.finish()
                for which, w in zip(outputs, expected):
                    np.testing.assert_array_equal(sampled(which).view(np.uint8), w.view(np.uint8))

            # the composite first, checked, then the operation (warm-up, and the call checked)
            composite()
            torch.cuda.synchronize()
            for which, w in zip(outputs, want):
                if which == "weights":
                    np.testing.assert_allclose(sampled(which), w, rtol=1e-6, atol=0)
                else:
                    np.testing.assert_array_equal(sampled(which).view(np.uint8), w.view(np.uint8))
            for which in outputs:
                t[which].zero_()
            op_flags()
            check(want_flags)
            assert (sampled("input_flags") & (OFF_TARGET | sum(MASK_BITS))).any()
            today()
            check(want_flags)
            op()
            check(want)
            yardstick()
            queue.finish()
            timed = time_rounds(queue, [op, composite, yardstick, op_flags, today], args.rounds,
                                args.calls)  # fmt: skip
            run = {"map": name, "weights": use_weights, "verified": True, "bytes": int(n_bytes),
                   "op": timed[0], "torch_composite": timed[1], "accumulate": timed[2],
                   "accumulate_bytes": int(samples * 35), "op_flags": timed[3],
                   "op_then_torch_flags": timed[4],
                   "flags_over_op": timed[3]["median_ms"] / timed[0]["median_ms"],
                   "today_over_flags": timed[4]["median_ms"] / timed[3]["median_ms"]}  # fmt: skip
            run["op"]["bytes_per_s"] = n_bytes / (timed[0]["median_ms"] * 1e-3)
            run["accumulate"]["bytes_per_s"] = samples * 35 / (timed[2]["median_ms"] * 1e-3)
            run["torch_over_op"] = timed[1]["median_ms"] / timed[0]["median_ms"]
            print(f"  weights={use_weights!s:5} {name:8}: op {text(timed[0])}, "
                  f"{run['op']['bytes_per_s'] / 1e12:.2f} TB/s; torch composite {text(timed[1])}, "
                  f"{run['torch_over_op']:.1f} x; Accumulate {text(timed[2])}, "
                  f"{run['accumulate']['bytes_per_s'] / 1e12:.2f} TB/s", flush=True)  # fmt: skip
            print(f"      with {CLASSES} classes + baseline flags: op {text(timed[3])}, "
                  f"{run['flags_over_op']:.3f} x the option-free op; option-free op + torch ORs "
                  f"{text(timed[4])}, {run['today_over_flags']:.2f} x", flush=True)  # fmt: skip
            result["runs"].append(run)
            del d_source, d_auto
        del op, op_flags, yardstick, t, masks_t, d_index, d_baseline_flags
        torch.cuda.empty_cache()
    if args.json:
        with open(args.json, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
