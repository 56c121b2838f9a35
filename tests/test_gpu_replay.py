"""-m gpu: the kernel calls the miniature models themselves make (one training step and one eval forward per miniature and arithmetic
mode: replay_util.LEGS), each distinct configuration replayed on the device against the fp64 emulator through gpu_cases.run_case,
storage-wide like the hand-written cases of tests/test_gpu_ops.py and at the bound those cases set for its precision class.  The legs
record on the CPU (the model lives there, every call on the emulator); only the replay uses the device."""
import collections
import os

import pytest
import torch

import parity_util
import replay_util as ru

REPORT = os.path.join(os.path.dirname(parity_util.REPORT), "replay_parity.txt")          # beside the full-size parity report


def _report(leg, rows):
    worst = collections.defaultdict(lambda: [0.0, 0.0])
    for entry, norm, elem in rows:
        worst[entry] = [max(worst[entry][0], norm), max(worst[entry][1], elem)]
    lines = [f"{entry:24s} {leg:44s} {n:9.3e} {e:9.3e}" for entry, (n, e) in sorted(worst.items())]
    print("\n".join(lines))
    try:
        os.makedirs(os.path.dirname(REPORT), exist_ok=True)
        with open(REPORT, "a") as f:
            f.write("\n".join(lines) + "\n")
    except OSError:
        pass


@pytest.mark.gpu
@pytest.mark.parametrize("leg", list(ru.LEGS))
def test_replayed_calls_match_the_emulator(leg):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    rec = ru.record_leg(leg)
    failures, rows = ru.replay(rec)
    _report(leg, rows)          # entry, leg, worst norm-wise error / bound, worst per-element error / bound
    assert not failures, f"{len(failures)} of {len(rec.snaps)} replayed calls fail:\n" + "\n".join(
        f"  {entry} at {site}\n    signature {sig}\n    {errs}" for entry, sig, site, errs in failures)
