"""CPU (`-m "not gpu"`): the 3ddet head's host side — factory wiring, the state-dict contract of the reference on mmcv 1.6.2, the
unsupported-option errors, and the plain-torch DCNv2 restatement the GPU tests compare against."""
import pytest
import torch
import torch.nn.functional as F

import conftest
import det_ref
from tests.golden import make_det_golden as mdg


def _cs_params():
    """TaskPrompter/configs/cityscapes3d/det_head_params.py (det_head_params + neck), as plain dicts"""
    p = det_ref.mini_head_params(in_channels=(450, 450, 450, 450), feat=256)        # neck widths = [final_embed_dim] * 4
    p.update(cls_branch=(256, 128))
    return p


def test_factory_builds_the_3ddet_head():
    import mtt_amd
    det_head, factory = mtt_amd.det_head, mtt_amd.factory
    p = factory.AttrDict(head='conv', mtt_prec='x3', det_head_params=_cs_params())
    head = factory.get_head(p, 256, '3ddet')
    assert isinstance(head, det_head.FCOS3DHead)
    assert head.prec.name == 'x3'
    assert mtt_amd.det_head is det_head


def test_state_dict_contract_matches_the_reference_layout():
    import mtt_amd
    det_head = mtt_amd.det_head
    head = det_head.FCOS3DHead(**_cs_params())
    sd = head.state_dict()
    shapes = {k: tuple(v.shape) for k, v in sd.items()}
    # FPN (ConvModule without norm: conv with bias)
    for i, c in enumerate((450, 450, 450, 450)):
        assert shapes[f'neck.lateral_convs.{i}.conv.weight'] == (256, c, 1, 1)
        assert shapes[f'neck.lateral_convs.{i}.conv.bias'] == (256,)
    for i in range(5):
        assert shapes[f'neck.fpn_convs.{i}.conv.weight'] == (256, 256, 3, 3)
    # towers: two plain ConvModules + the DCNv2 layer (ModulatedDeformConv2dPack under `.conv`)
    for tower in ('cls_convs', 'reg_convs'):
        for i in range(2):
            assert shapes[f'{tower}.{i}.conv.weight'] == (256, 256, 3, 3)
            assert shapes[f'{tower}.{i}.conv.bias'] == (256,)
            assert shapes[f'{tower}.{i}.gn.weight'] == (256,) and shapes[f'{tower}.{i}.gn.bias'] == (256,)
        assert shapes[f'{tower}.2.conv.weight'] == (256, 256, 3, 3)
        assert shapes[f'{tower}.2.conv.bias'] == (256,)
        assert shapes[f'{tower}.2.conv.conv_offset.weight'] == (27, 256, 3, 3)
        assert shapes[f'{tower}.2.conv.conv_offset.bias'] == (27,)
    assert list(k for k in sd if k.startswith('cls_convs.2.')) == [
        'cls_convs.2.conv.weight', 'cls_convs.2.conv.bias', 'cls_convs.2.conv.conv_offset.weight', 'cls_convs.2.conv.conv_offset.bias',
        'cls_convs.2.gn.weight', 'cls_convs.2.gn.bias']
    assert shapes['conv_cls_prev.1.conv.weight'] == (128, 256, 3, 3) and shapes['conv_cls_prev.1.gn.weight'] == (128,)
    assert shapes['conv_cls.weight'] == (6, 128, 1, 1)
    for g, n in enumerate((2, 1, 3, 3, 4)):
        assert shapes[f'conv_reg_prevs.{g}.0.conv.weight'] == (256, 256, 3, 3)
        assert shapes[f'conv_regs.{g}.weight'] == (n, 256, 1, 1)
    assert shapes['conv_dir_cls_prev.0.gn.bias'] == (256,) and shapes['conv_dir_cls.weight'] == (6, 256, 1, 1)
    assert shapes['conv_centerness_prev.0.conv.weight'] == (256, 256, 3, 3) and shapes['conv_centerness.weight'] == (1, 256, 1, 1)
    for lv in range(5):
        for j in range(4):
            assert shapes[f'scales.{lv}.{j}.scale'] == ()
    assert not any('activate' in k for k in sd)
    # a state dict of this layout loads strictly
    head2 = det_head.FCOS3DHead(**_cs_params())
    head2.load_state_dict(sd, strict=True)


@pytest.mark.parametrize("bad", [
    dict(pred_keypoints=True),
    dict(neck_cfg=dict(_cs_params()['neck_cfg'], add_extra_convs='on_input')),
    dict(neck_cfg=dict(_cs_params()['neck_cfg'], norm_cfg=dict(type='GN', num_groups=32))),
    dict(norm_cfg=dict(type='BN')),
])
def test_unsupported_options_raise(bad):
    import mtt_amd
    det_head = mtt_amd.det_head
    with pytest.raises(NotImplementedError):
        det_head.FCOS3DHead(**dict(_cs_params(), **bad))


def test_dcn_without_dcn_on_last_conv_builds_plain_towers():
    import mtt_amd
    det_head = mtt_amd.det_head
    head = det_head.FCOS3DHead(**dict(_cs_params(), dcn_on_last_conv=False))
    assert isinstance(head.cls_convs[2].conv, torch.nn.Conv2d)
    assert 'cls_convs.2.conv.conv_offset.weight' not in head.state_dict()


def test_dcn_restatement_matches_a_brute_force_loop():
    torch.manual_seed(0)
    B, C, Co, H, W = 2, 5, 4, 6, 7
    x = torch.randn(B, C, H, W, dtype=torch.float64)
    w = torch.randn(Co, C, 3, 3, dtype=torch.float64)
    b = torch.randn(Co, dtype=torch.float64)
    for stride in (1, 2):
        Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
        off = 3.0 * torch.randn(B, 18, Ho, Wo, dtype=torch.float64)         # many samples leave the map
        mask = torch.rand(B, 9, Ho, Wo, dtype=torch.float64)
        mask[:, 4] = 0.0
        y = det_ref.dcn_v2(x, off, mask, w, b, stride=stride)
        assert torch.allclose(y, det_ref.dcn_brute(x, off, mask, w, b, stride=stride), atol=1e-12)
        # no offsets, mask 0.5: the plain (strided) conv scaled by one half
        y0 = det_ref.dcn_v2(x, None, torch.full((B, 9, Ho, Wo), 0.5, dtype=torch.float64), w, None, stride=stride)
        assert torch.allclose(y0, 0.5 * F.conv2d(x, w, None, stride=stride, padding=1), atol=1e-12)


def _fixture():
    import numpy as np
    meta, arrs = conftest.load_golden("mini_det")
    return meta, {k: torch.from_numpy(np.asarray(v)) for k, v in arrs.items()}


def _fixture_head():
    import mtt_amd
    torch.manual_seed(0)
    head = mtt_amd.det_head.FCOS3DHead(**det_ref.mini_head_params())
    head.init_weights()
    det_ref.randomize(head, 0)
    return head


def test_state_dict_contract_equals_the_reference_fixture():
    """names, shapes and ORDER of the product's state dict == the unmodified reference's (tests/golden/mini_det.json); its weights load
    into a second product head with strict=True"""
    meta, _ = _fixture()
    head = _fixture_head()
    assert [(k, list(v.shape)) for k, v in head.state_dict().items()] == [(k, list(s)) for k, s in meta["contract"]]
    import mtt_amd
    other = mtt_amd.det_head.FCOS3DHead(**det_ref.mini_head_params())
    other.load_state_dict(head.state_dict(), strict=True)


def test_restatement_reproduces_the_reference_fixture():
    """the plain-torch restatement the GPU tests use (det_ref.head_forward) on the fixture's weights and inputs == the reference's outputs"""
    meta, arrs = _fixture()
    head = _fixture_head()
    feats = [arrs[f"in{i}"] for i in range(4)]
    outs = [t for lst in det_ref.head_forward(head, feats) for t in lst]
    assert len(outs) == 20
    for i, o in enumerate(outs):
        r = arrs[f"out{i}"]
        assert o.shape == r.shape
        assert float((o - r).norm() / r.norm()) < 1e-5, i


def test_reference_regenerates_the_fixture(tmp_path):
    """the stand-in + the unmodified reference files reproduce tests/golden/mini_det.* byte for byte (build container only; a child process,
    so that the stand-in `mmcv` never enters this interpreter's modules)"""
    import os
    import subprocess
    import sys
    if not os.path.isdir(os.path.join(mdg.REF, "TaskPrompter", "detection_toolbox")):
        pytest.skip("reference tree not present")
    r = subprocess.run([sys.executable, mdg.__file__, str(tmp_path)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    for name in ("mini_det.json", "mini_det.npz"):
        assert open(tmp_path / name, "rb").read() == open(os.path.join(conftest.GOLDEN, name), "rb").read(), name


def test_get_model_refuses_3ddet_until_the_backbone_is_wired():
    import mtt_amd
    p = mtt_amd.factory.make_p(["semseg", "depth", "3ddet"], (64, 128), backbone="TaskPrompter_swinB",
                               num_output={"3ddet": 1}, det_head_params=det_ref.mini_head_params())
    with pytest.raises(NotImplementedError):
        mtt_amd.factory.get_model(p)
