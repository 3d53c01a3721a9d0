#!/usr/bin/env python3
"""Time the Python of one call of a bound, lean ``FusedFlaggerDevice`` on the fake backend of
``tests/fakes.py``: no GPU, the kernel launch is a no-op, so what is left is the host path the
benchmark pays per step (``Operation.__call__``, ``FusedFlaggerDevice._run``, building the
argument list). A guard for changes to that path; to compare two trees, run the copy of this
file in each, alternately. Prints one JSON line. Usage:
``python tools/time_fused_call_fake.py [--calls N]``.
"""

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from katsdpsigproc_amd import tune  # noqa: E402
from katsdpsigproc_amd.rfi import device  # noqa: E402
from tests.fakes import FakeContext  # noqa: E402


class _Discard(list):
    """``FakeQueue.launches`` that keeps nothing: 200000 recorded launches would be timed too."""

    def append(self, item):
        pass


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--calls", type=int, default=200000)
    args = parser.parse_args()
    tune.autotuner_impl = tune.stub_autotuner
    context = FakeContext()
    queue = context.create_command_queue()
    template = device.FlaggerDeviceTemplate(
        device.BackgroundMedianFilterDeviceTemplate(context, 13),
        device.NoiseEstMADTDeviceTemplate(context, 10240),
        device.ThresholdSumDeviceTemplate(context),
    )
    fn = template.instantiate(queue, 4096, 64, threshold_args={"n_sigma": 11.0})
    assert isinstance(fn, device.FusedFlaggerDevice)
    fn.ensure_all_bound()
    queue.launches = _Discard()
    for _ in range(args.calls // 10):
        fn()
    start = time.perf_counter()
    for _ in range(args.calls):
        fn()
    elapsed = time.perf_counter() - start
    print(json.dumps({"calls": args.calls, "us_per_call": round(elapsed / args.calls * 1e6, 4)}))


if __name__ == "__main__":
    main()
