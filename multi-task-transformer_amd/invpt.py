"""MI355X-native InvPT: same nn.Module API / state_dict layout as the reference
(InvPT/models/transformers/vit.py, transformer_decoder.py, invpt.py, InvPT/models/transformer_net.py),
executed on the libmtt_hip.so kernels.

Schedule (differs from the reference's op graph):
  * ViT: one fp32 token buffer [B, 1+hw, C] (cls first), LayerNorm -> qkv GEMM -> flash attention -> proj GEMM
    (+residual) -> LayerNorm -> fc1+GELU -> fc2 (+residual); taps are copies of the patch rows.
  * Decoder feature maps are task-major NHWC stacks [T, B*g*g, pitch(D)]; every per-task conv / BN / 1x1 is one
    task-batched launch; the shared-weight Linears (proj_q/k/v, proj, MLP) run once over all tasks' tokens.
  * Cross-task attention (heads = 2, head dim D/2 not 64) uses the batched GEMM + row-softmax kernels on
    batch-major q/k/v ([B, T*q, .]) that the projection GEMMs produce through their row-group output mapping
    (with gradients: BLinearFn + a permuted copy); heads are padded to 8-column multiples.  The message passing of
    invpt.py:208-229 is one fused kernel.
  * Dead reference compute is skipped (scale_embed[2], norm_mt, stage-0 fuse_attn, redu_chan[0]); their parameters
    exist (strict state_dict) and — as in the reference — receive no gradient.

This file holds the modules (parameter holders with the reference's names and shapes) and the reference-API entry points; they compute
`keep` (will somebody differentiate the result?) and call the one forward in invpt_autograd.py: vit_taps, decoder_forward, net_forward.
"""
from collections import OrderedDict
from functools import partial

import torch
import torch.nn as nn

from . import ops
from .taskprompter import Mlp, PatchEmbed, _init_vit_weights, _prec_of, trunc_normal_

BATCHNORM = nn.SyncBatchNorm      # invpt.py:14, transformer_decoder.py:13 (parameter holder; statistics are computed by the kernels)
pitch = ops.pitch


# ---------------------------------------------------------------------------------------------------------
# ViT backbone (vit.py:172-351)
# ---------------------------------------------------------------------------------------------------------
class Attention(nn.Module):
    def __init__(self, dim, num_heads=8, qkv_bias=False):
        super().__init__()
        self.num_heads = num_heads
        self.qkv = nn.Linear(dim, dim * 3, bias=qkv_bias)
        self.proj = nn.Linear(dim, dim)


class Block(nn.Module):
    def __init__(self, dim, num_heads, mlp_ratio=4., qkv_bias=False, drop_path=0., norm_layer=nn.LayerNorm):
        super().__init__()
        self.norm1 = norm_layer(dim)
        self.attn = Attention(dim, num_heads=num_heads, qkv_bias=qkv_bias)
        self.drop_path_rate = float(drop_path)
        self.norm2 = norm_layer(dim)
        self.mlp = Mlp(dim, int(dim * mlp_ratio))


class VisionTransformer(nn.Module):
    """vit.py:218-351; forward(x) -> (x_last [B, hw, C], [4 taps [B, hw, C]])."""

    def __init__(self, select_list, img_size=224, patch_size=16, in_chans=3, num_classes=1000, embed_dim=768, depth=12,
                 num_heads=12, mlp_ratio=4., qkv_bias=True, representation_size=None, distilled=False, drop_rate=0.,
                 attn_drop_rate=0., drop_path_rate=0., embed_layer=None, norm_layer=None, act_layer=None, weight_init='',
                 prec=ops.DEFAULT_PREC):
        super().__init__()
        assert patch_size == 16 and embed_dim // num_heads == 64 and not distilled
        self.num_features = self.embed_dim = embed_dim
        self.num_heads = num_heads
        norm_layer = norm_layer or partial(nn.LayerNorm, eps=1e-6)
        if isinstance(img_size, int):
            img_size = (img_size, img_size)
        self.patch_embed = PatchEmbed(img_size=img_size, patch_size=patch_size, in_chans=in_chans, embed_dim=embed_dim)
        self.cls_token = nn.Parameter(torch.zeros(1, 1, embed_dim))
        self.pos_embed = nn.Parameter(torch.zeros(1, self.patch_embed.num_patches + 1, embed_dim))
        dpr = [x.item() for x in torch.linspace(0, drop_path_rate, depth)]
        self.blocks = nn.Sequential(*[Block(embed_dim, num_heads, mlp_ratio, qkv_bias, dpr[i], norm_layer) for i in range(depth)])
        self.norm = norm_layer(embed_dim)
        self.select_list = list(select_list)
        trunc_normal_(self.pos_embed, std=.02)
        trunc_normal_(self.cls_token, std=.02)
        self.apply(_init_vit_weights)
        self.prec = ops.Prec(prec)

    def load_pretrained(self, checkpoint_path, prefix=''):
        """vit.py:320-321: import a Google/Flax ViT .npz (class token, resized position embedding)."""
        from .checkpoints import load_flax_vit_npz
        return load_flax_vit_npz(self, checkpoint_path, prefix)

    def forward(self, img):
        taps = self.forward_taps(img)
        B = img.shape[0]
        return taps[-1].view(B, -1, self.embed_dim).float(), [t.view(B, -1, self.embed_dim).float() for t in taps]

    def forward_taps(self, img):
        """-> 4 contiguous [B*hw, C] activation-dtype token maps (cls dropped), vit.py:340-349."""
        from . import invpt_autograd
        keep = torch.is_grad_enabled() and (img.requires_grad or any(q.requires_grad for q in self.parameters()))
        return invpt_autograd.vit_taps(self, img, keep)


def _create_vision_transformer(variant, pretrained=False, default_cfg=None, **kwargs):
    kwargs.pop('representation_size', None)
    model = VisionTransformer(**kwargs)
    model.default_cfg = dict(default_cfg or {}, variant=variant)
    if pretrained:                       # vit.py:541: from the torch hub cache only (checkpoints.load_cached_pretrained), never the network
        from .checkpoints import load_cached_pretrained
        load_cached_pretrained(model, variant)
    return model


def vit_large_patch16_384(pretrained=False, **kwargs):
    """ViT-L/16 (vit.py:556-562)."""
    model_kwargs = dict(select_list=[6, 12, 18], patch_size=16, embed_dim=1024, depth=24, num_heads=16, **kwargs)
    return _create_vision_transformer('vit_large_patch16_384', pretrained=pretrained, **model_kwargs)


# ---------------------------------------------------------------------------------------------------------
# Decoder parameter holders (names / shapes of transformer_decoder.py and invpt.py)
# ---------------------------------------------------------------------------------------------------------
class UpEmbed(nn.Module):
    def __init__(self, in_chans, embed_dim):
        super().__init__()
        self.proj = nn.Sequential(nn.Upsample(scale_factor=2, mode='bilinear', align_corners=False),
                                  nn.Conv2d(in_chans, embed_dim, 3, padding=2, stride=1, bias=False, dilation=2), BATCHNORM(embed_dim),
                                  nn.ReLU(inplace=True),
                                  nn.Conv2d(embed_dim, embed_dim, 3, padding=2, stride=1, bias=False, dilation=2), BATCHNORM(embed_dim),
                                  nn.ReLU(inplace=True))


class InvPTMlp(nn.Module):
    def __init__(self, dim, hidden):
        super().__init__()
        self.fc1 = nn.Linear(dim, hidden)
        self.fc2 = nn.Linear(hidden, dim)


class SelfAttention(nn.Module):
    def __init__(self, fea_no, dim, num_heads, qkv_bias=True):
        super().__init__()
        self.num_heads, self.dim, self.fea_no = num_heads, dim, fea_no
        self.conv_proj_q = nn.ModuleList([nn.Sequential(OrderedDict([
            ('conv', nn.Conv2d(dim, dim, 3, padding=1, stride=2, bias=False, groups=dim)), ('bn', BATCHNORM(dim))]))
            for _ in range(fea_no)])
        self.proj_q = nn.Linear(dim, dim, bias=qkv_bias)
        self.proj_k = nn.Linear(dim, dim, bias=qkv_bias)
        self.proj_v = nn.Linear(dim, dim, bias=qkv_bias)
        self.proj = nn.Linear(dim, dim)
        self.fuse_attn = nn.Conv2d(num_heads * 2, num_heads, 1)


class InvPTBlock(nn.Module):
    def __init__(self, task_no, dim, num_heads, mlp_ratio=4.):
        super().__init__()
        self.norm1 = nn.LayerNorm(dim)
        self.norm2 = nn.LayerNorm(dim)
        self.mlp = InvPTMlp(dim, int(dim * mlp_ratio))
        self.attn = SelfAttention(task_no, dim, num_heads)


def _init_trunc(m):
    if isinstance(m, nn.Linear):
        trunc_normal_(m.weight, std=0.02)
        if m.bias is not None:
            nn.init.constant_(m.bias, 0)
    elif isinstance(m, (nn.LayerNorm, nn.modules.batchnorm._BatchNorm)):
        nn.init.constant_(m.bias, 0)
        nn.init.constant_(m.weight, 1.0)


class InvPTStage(nn.Module):
    def __init__(self, task_no, stage_idx, in_chans, embed_dim, num_heads):
        super().__init__()
        self.stage_idx = stage_idx
        self.patch_embed = None if stage_idx == 0 else nn.ModuleList([UpEmbed(in_chans, embed_dim) for _ in range(task_no)])
        self.blocks = nn.ModuleList([InvPTBlock(task_no, embed_dim, num_heads)])
        self.apply(_init_trunc)


class InvPT(nn.Module):
    def __init__(self, p, in_chans, spec):
        super().__init__()
        self.p = p
        self.all_tasks = p.TASKS.NAMES
        T = len(self.all_tasks)
        self.norm_mts = nn.ModuleList()
        self.redu_chan = nn.ModuleList()
        self.invpt_stages = nn.ModuleList()
        self.mt_embed_dims = []
        cur = in_chans
        for i in range(spec['NUM_STAGES']):
            d = spec['DIM_EMBED'][i]
            self.invpt_stages.append(InvPTStage(T, i, cur, d, spec['NUM_HEADS'][i]))
            cur = d
            self.norm_mts.append(nn.LayerNorm(d * T))
            self.mt_embed_dims.append(d)
            self.redu_chan.append(nn.ModuleList([nn.Conv2d(d, in_chans, 1) for _ in range(T)]))
        self.norm_mt = nn.LayerNorm(T * cur)
        self.mt_proj = nn.ModuleDict()
        for task in self.all_tasks:
            self.mt_proj[task] = nn.Sequential(nn.Conv2d(in_chans, in_chans, 3, padding=1), BATCHNORM(in_chans), nn.ReLU(True))
            trunc_normal_(self.mt_proj[task][0].weight, std=0.02)
        self.mix_proj = nn.ModuleDict()
        for t in self.all_tasks:
            self.mix_proj[t] = nn.Sequential(nn.Conv2d(spec['ori_embed_dim'] + p.TASKS.NUM_OUTPUT[t], in_chans, 1))


class ConvBlock(nn.Module):
    def __init__(self, inplanes, planes):
        super().__init__()
        self.conv = nn.Conv2d(inplanes, planes, kernel_size=3, stride=1, padding=1, bias=False)
        self.bn1 = BATCHNORM(planes)
        self.relu = nn.ReLU(inplace=True)


class MLPHead(nn.Module):
    """transformer_decoder.py:124-131."""

    def __init__(self, in_channels, num_classes):
        super().__init__()
        self.linear_pred = nn.Conv2d(in_channels, num_classes, kernel_size=1)


class TransformerDecoder(nn.Module):
    """transformer_decoder.py:18-98 + InvPT.forward (invpt.py:502-544)."""

    def __init__(self, p):
        super().__init__()
        self.embed_dim = p.embed_dim
        E = self.embed_dim + p.PRED_OUT_NUM_CONSTANT
        p.mtt_resolution = [_ // p.mtt_resolution_downsample_rate for _ in p.spatial_dim[-1]]
        self.p = p
        spec = dict(ori_embed_dim=self.embed_dim, NUM_STAGES=3, DIM_EMBED=[E, E // 2, E // 4], NUM_HEADS=[2, 2, 2])
        input_channels = p.backbone_channels[-1]
        self.intermediate_head = nn.ModuleDict()
        self.invpt = InvPT(p, in_chans=E, spec=spec)
        self.preliminary_decoder = nn.ModuleDict()
        for t in p.TASKS.NAMES:
            self.intermediate_head[t] = nn.Conv2d(self.embed_dim, p.TASKS.NUM_OUTPUT[t], 1)
            self.preliminary_decoder[t] = nn.Sequential(ConvBlock(input_channels, input_channels), ConvBlock(input_channels, self.embed_dim))
        self.scale_embed = nn.ModuleList()
        self.scale_embed.append(nn.ConvTranspose2d(p.backbone_channels[0], E // 4, kernel_size=3, stride=2, padding=1, output_padding=1))
        self.scale_embed.append(nn.Conv2d(p.backbone_channels[1], E // 2, 3, padding=1))
        self.scale_embed.append(nn.Conv2d(p.backbone_channels[2], E, 3, padding=1))
        self.scale_embed.append(None)
        self.prec = _prec_of(p)

    # -------------------------------------------------------------------------------------------------
    def forward(self, x_list):
        """x_list: 4 token maps [B, hw, C] (reference API) -> ({task: [B, E, 8mh, 8mw]}, {task: [B, n, mh, mw]})."""
        B = x_list[0].shape[0]
        taps = [t.reshape(-1, t.shape[-1]).to(self.prec.adt).contiguous() for t in x_list]
        feats, inter = self.forward_nhwc(taps, B)
        names, p = self.p.TASKS.NAMES, self.p
        mh, mw = p.mtt_resolution
        E = self.embed_dim + p.PRED_OUT_NUM_CONSTANT
        out = {t: feats[i].view(B, 8 * mh, 8 * mw, -1)[..., :E].permute(0, 3, 1, 2).float() for i, t in enumerate(names)}
        ip = {t: inter[t].view(B, mh, mw, -1)[..., :p.TASKS.NUM_OUTPUT[t]].permute(0, 3, 1, 2).float() for t in names}
        return out, ip

    def forward_nhwc(self, taps, B):
        """taps: 4 contiguous [B*hw, C] maps.  -> (features [T, B*8mh*8mw, pitch(E)], {task: inter_pred [B*mh*mw, pitch(n)] fp32})."""
        from . import invpt_autograd
        keep = torch.is_grad_enabled() and (any(t.requires_grad for t in taps) or any(q.requires_grad for q in self.parameters()))
        f, inter = invpt_autograd.decoder_forward(self, taps, B, keep)
        return f, {t: v[0] for t, v in inter.items()}


class TransformerNet(nn.Module):
    """transformer_net.py:13-38."""

    def __init__(self, p, backbone, backbone_channels, heads):
        super().__init__()
        self.tasks = p.TASKS.NAMES
        self.backbone = backbone
        self.multi_task_decoder = TransformerDecoder(p)
        self.heads = heads
        self.p = p

    def forward(self, x):
        from . import invpt_autograd
        keep = torch.is_grad_enabled() and (x.requires_grad or any(q.requires_grad for q in self.parameters()))
        return invpt_autograd.net_forward(self, x, keep)
