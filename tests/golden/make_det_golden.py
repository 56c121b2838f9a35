"""Golden fixture of the 3ddet head (FPN + FCOS3DHead), generated from the UNMODIFIED reference files
TaskPrompter/detection_toolbox/det_head.py and fpn.py in the build container:

    python tests/golden/make_det_golden.py    ->  tests/golden/mini_det.json, tests/golden/mini_det.npz

mmcv / termcolor are absent: tests/det_refshim stands in for them with the restated layers (ConvModule, ModulatedDeformConv2dPack,
BaseModule, Registry, auto_fp16, colored) — the only part of the computation that is not the reference's own code.  The head is the
cs_swinB structure at miniature width (tests/det_ref.mini_head_params: FPN / feature width 64, GN 32 groups, cls_branch (64, 32) = one
channel per group, dcn_on_last_conv=True, stacked_convs 3, num_outs 5), weights from det_ref.randomize (DCN offsets of about +-3 px,
samples outside the map; GN affine parameters and Scales randomised).  Stored: the state-dict contract (names, shapes, order), the inputs,
the 20 eval outputs, and per parameter the norm and a fixed random projection of the gradient of loss = sum_i <out_i, proj_i>."""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
REF = os.environ.get("MTT_REFERENCE_ROOT", "/root/reference")
LEVELS = ((32, 12, 20), (48, 6, 10), (64, 3, 5), (64, 3, 5))
B = 2


def inputs():
    g = torch.Generator().manual_seed(5)
    return [torch.randn(B, c, h, w, generator=g) for c, h, w in LEVELS]


def projections(outs):
    g = torch.Generator().manual_seed(9)
    return [torch.randn(t.shape, generator=g) for t in outs]


def grad_probe(name, shape):
    """the fixed random direction a parameter's gradient is projected on"""
    g = torch.Generator().manual_seed(sum(ord(c) * (i + 1) for i, c in enumerate(name)) % (2 ** 31))
    return torch.randn(shape, generator=g, dtype=torch.float64)


def grad_stats(named_grads):
    return {k: (float(g.double().norm()), float((g.double().cpu() * grad_probe(k, g.shape)).sum())) for k, g in named_grads}


def reference_head():
    for p in (os.path.join(TESTS, "det_refshim"), TESTS, os.path.join(REF, "TaskPrompter")):
        if p not in sys.path:
            sys.path.insert(0, p)
    import det_ref
    from detection_toolbox import fpn  # noqa: F401  (registers FPN with the NECKS registry)
    from detection_toolbox.det_head import FCOS3DHead
    torch.manual_seed(0)
    head = FCOS3DHead(**det_ref.mini_head_params())
    head.init_weights()
    det_ref.randomize(head, 0)
    return head


def generate():
    torch.set_num_threads(1)
    head = reference_head()
    feats = inputs()
    head.eval()
    outs = [t for lst in head(feats) for t in lst]
    loss = sum((o * p).sum() for o, p in zip(outs, projections(outs)))
    loss.backward()
    contract = [(k, list(v.shape)) for k, v in head.state_dict().items()]
    stats = grad_stats((k, p.grad) for k, p in head.named_parameters())
    arrays = {f"in{i}": f.numpy() for i, f in enumerate(feats)}
    arrays.update({f"out{i}": o.detach().numpy() for i, o in enumerate(outs)})
    return contract, stats, arrays


def main(out_dir=HERE):
    contract, stats, arrays = generate()
    with open(os.path.join(out_dir, "mini_det.json"), "w") as f:
        json.dump({"contract": contract, "grad_stats": stats, "levels": LEVELS, "batch": B}, f, indent=0, sort_keys=True)
    np.savez_compressed(os.path.join(out_dir, "mini_det.npz"), **arrays)


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else HERE)       # an output directory other than tests/golden: a regeneration check
