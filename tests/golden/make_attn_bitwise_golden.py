"""Generate tests/golden/attn_bitwise.json: sha256 digests of what the flash-attention kernels (forward, dQ, dK/dV) write on the 16 ragged
shapes of tests/attn_bitwise_util.py, for inputs drawn on the CPU from a seeded generator.

Run from the repository root on an MI355X:
    python tests/golden/make_attn_bitwise_golden.py [--kernel "which kernels these are"]
The committed file was NOT recorded from the kernels it now guards: it holds the outputs of the register-staged generation of the kernels
(mtt_attn_desc.variant = 3 at the commit named in the file, the last one that had it), an independently staged implementation with the
same arithmetic order, which the LDS-DMA kernels matched bit for bit there.  Re-recording from the current kernels is right only when a
change to their arithmetic order is intended; say so in "kernel".
"""
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import attn_bitwise_util as abu  # noqa: E402


def record(device="cuda"):
    """{shape id: {"inputs": digest, "out": ..., "rawlog": ..., "lse": ..., "dqkv": ..., "stat": ...}} from one forward and one backward"""
    import mtt_amd  # noqa: F401
    res = {}
    for shape in abu.SHAPES:
        inputs = abu.make_inputs(shape, device)
        fwd = abu.forward(shape, inputs)
        res[abu.shape_id(shape)] = dict(inputs=abu.inputs_digest(inputs), **abu.digests(fwd, abu.backward(shape, inputs, fwd)))
    return res


def provenance(kernel):
    def out(cmd):
        try:
            return subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT).stdout.strip()
        except OSError:
            return ""
    hipcc = out([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "--version"]).splitlines()
    return dict(commit=out(["git", "rev-parse", "HEAD"]) or None, compiler=" / ".join(ln for ln in hipcc[:2]), kernel=kernel)


def write(shapes, prov, path=abu.GOLDEN):
    with open(path, "w") as f:
        json.dump(dict(recorded_on=prov, shapes=shapes), f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    kernel = sys.argv[sys.argv.index("--kernel") + 1] if "--kernel" in sys.argv else "the library's flash kernels (default dispatch)"
    write(record(), provenance(kernel))
    print("wrote", abu.GOLDEN)
