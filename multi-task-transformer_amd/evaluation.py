"""Validation on the device: the reference's `get_output` (TaskPrompter/utils/utils.py:27-63) and task meters
(TaskPrompter/evaluation/eval_*.py, evaluate_utils.py:13-66; InvPT/evaluation) on the HIP kernels of csrc/eval_ops.hip.

`get_output(output, task)` returns the same maps as the reference.  Every meter keeps its running statistics in one small device
buffer (int64 counts, fp64 sums) and has two ways in:

    meter.update(get_output(output[t], t), gt[t])      # what the reference's test_phase does
    meter.update_from_logits(output[t], gt[t])         # fused: one pass over the logits, no map is written

Both feed the same per-pixel values into the same kernel code and give bitwise equal states.  Neither synchronises with the host, so
a whole validation batch is capturable in a hipGraph (run one update, or `meter.to(device)` plus one update, before capturing: the
accumulator, the thresholds and the reduction workspace are allocated on first use).  `state()` is the one device-to-host copy;
`get_score` takes it once and repeats the reference's host arithmetic.

There is no fallback: CPU tensors and logits that are not fp32 raise RuntimeError.

Differences from the reference, all deliberate:
  * SaliencyMeter counts in exact int64 where the reference accumulates float32 tensors; the two are identical while every counter is
    below 2**24.  Its quirk of applying `torch.sigmoid` to the map / 255 (a probability, not a logit) is reproduced.
  * EdgeMeter treats a batch of one like any other; the reference raises IndexError there (`gt.squeeze()` drops the batch axis).  It
    accumulates the per-pixel balanced-BCE terms, where the reference multiplies each batch's float32 mean back by its pixel count.
  * DepthMeter.update does not write 1e-9 into the caller's `pred` and `gt` (the reference does, in place).  `get_output(.., 'depth')`
    does clamp the caller's tensor in place, like the reference.
  * As in the reference, get_score of DepthMeter, NormalsMeter and EdgeMeter raises ZeroDivisionError while no valid pixel has been
    seen (each divides by its pixel count, a Python number); the confusion and saliency meters return 0.
  * `reset()` exists on every meter.  HumanPartsMeter.get_score prints only when `verbose`.
  * Class names are not built in: pass `cat_names=[...]` to get_score, indices are printed otherwise.
"""
import numpy as np
import torch

from . import _lib

TASKS_2D = ('semseg', 'human_parts', 'normals', 'edge', 'sal', 'depth')
CS_VALID_CLASSES = (7, 8, 11, 12, 13, 17, 19, 20, 21, 22, 23, 24, 25, 26, 27, 28, 31, 32, 33)     # Cityscapes train id -> label id

_MAP_KIND = dict(semseg=_lib.EVAL_CONFUSION, human_parts=_lib.EVAL_CONFUSION, sal=_lib.EVAL_SAL, depth=_lib.EVAL_DEPTH,
                 normals=_lib.EVAL_NORMALS, edge=_lib.EVAL_EDGE)
_class_maps = {}


def _call(name, **kw):
    from . import ops
    return ops.call(name, **kw)


def _logits(output, what="logits"):
    if not isinstance(output, torch.Tensor) or not output.is_cuda:
        raise RuntimeError("%s must be a tensor on a HIP device (evaluation has no CPU fallback)" % what)
    if output.dtype != torch.float32:
        raise RuntimeError("%s must be fp32, as the model wrappers return them (got %s)" % (what, output.dtype))
    if output.dim() != 4:
        raise RuntimeError("%s must be [B, C, H, W] (got %s)" % (what, tuple(output.shape)))
    return output


def _label(gt, B, Cl, HW, device):
    if not isinstance(gt, torch.Tensor) or not gt.is_cuda:
        raise RuntimeError("labels must be a tensor on a HIP device (evaluation has no CPU fallback)")
    if gt.device != device:
        raise RuntimeError("labels are on %s, predictions on %s" % (gt.device, device))
    if gt.numel() != B * Cl * HW or gt.shape[0] != B:
        raise RuntimeError("labels of shape %s do not match %d images of %d x %d values" % (tuple(gt.shape), B, Cl, HW))
    return gt.float().contiguous()


def get_output(output, task, p=None, label=None, semseg_save_train_class=True):
    """utils.py:27-63.  semseg / human_parts: int64 [B, H, W] arg-max (first index wins ties; with semseg_save_train_class=False the
    Cityscapes label ids); normals: fp32 [B, H, W, 3]; edge, sal: fp32 [B, H, W]; depth: `output` clamped at 0 IN PLACE and returned as
    its [B, H, W, 1] view; 3ddet: p.detmodel.get_results_from_bbox(output, label, rescale=False)."""
    if task == '3ddet':
        return p.detmodel.get_results_from_bbox(output, label, rescale=False)
    if task not in _MAP_KIND:
        raise ValueError('Select one of the valid tasks')
    x = _logits(output)
    B, C, H, W = x.shape
    kind = _MAP_KIND[task]
    cmap = None
    if task == 'depth':
        if not x.is_contiguous():
            raise RuntimeError("get_output('depth') clamps its argument in place and needs it contiguous")
        out = x
    else:
        x = x.contiguous()
        if kind == _lib.EVAL_CONFUSION:
            out = torch.empty(B, H, W, dtype=torch.int64, device=x.device)
            if task == 'semseg' and not semseg_save_train_class:
                cmap = _class_maps.get(x.device)
                if cmap is None:
                    cmap = _class_maps[x.device] = torch.tensor(CS_VALID_CLASSES, dtype=torch.int64, device=x.device)
        elif kind == _lib.EVAL_NORMALS:
            out = torch.empty(B, H, W, 3, dtype=torch.float32, device=x.device)
        else:
            out = torch.empty(B, H, W, dtype=torch.float32, device=x.device)
    _call("eval_map", pred=x, out=out, class_map=cmap, n_map=0 if cmap is None else cmap.numel(), B=B, HW=H * W, C=C, kind=kind)
    return out.permute(0, 2, 3, 1) if task == 'depth' else out


class _Meter(object):
    """Device accumulator shared by the meters: `_slots` 8-byte slots, int64 and fp64 mixed as include/mtt_hip.h lays them out."""
    _kind = None
    _map_dtype = torch.float32
    _channels = None           # logits channels the kernel takes (None: any)
    _label_channels = 1

    def _init_state(self, slots):
        self._slots = int(slots)
        self._acc = None
        self._ws = {}
        self._extra = {}

    def _fields(self, device):
        return {}

    def to(self, device):
        """Allocate (or move) the accumulator on `device`; update does it on first use otherwise."""
        device = torch.device(device)
        if device.type != 'cuda':
            raise RuntimeError("meters accumulate on a HIP device (no CPU fallback)")
        if device.index is None:
            device = torch.device('cuda', torch.cuda.current_device())
        if self._acc is None:
            self._acc = torch.zeros(self._slots, dtype=torch.int64, device=device)
        elif self._acc.device != device:
            self._acc = self._acc.to(device)
            self._ws, self._extra = {}, {}
        return self

    def reset(self):
        if self._acc is not None:
            self._acc.zero_()          # in place: a captured graph keeps adding to the same buffer

    def _accum(self, pred, gt, source, B, C, HW):
        self.to(pred.device)
        label = _label(gt, B, self._label_channels, HW, pred.device)
        n = _lib.eval_ws_floats(self._kind, B, HW)
        ws = None
        if n:
            ws = self._ws.get(n)
            if ws is None:
                ws = self._ws[n] = torch.empty(n // 2, dtype=torch.float64, device=pred.device)
        _call("eval_accum", pred=pred, label=label, acc=self._acc, ws=ws, B=B, HW=HW, C=C, Cl=self._label_channels, kind=self._kind,
              source=source, **self._fields(pred.device))

    @torch.no_grad()
    def update_from_logits(self, output, gt):
        """One batch straight from the logits [B, C, H, W]: the same statistics as update(get_output(output, task), gt), bitwise."""
        x = _logits(output).contiguous()
        B, C, H, W = x.shape
        if self._channels is not None and C != self._channels:
            raise RuntimeError("%s takes %d-channel logits (got %d)" % (type(self).__name__, self._channels, C))
        self._accum(x, gt, _lib.EVAL_FROM_LOGITS, B, C, H * W)

    @torch.no_grad()
    def update(self, pred, gt):
        """One batch from the map get_output returned."""
        if not isinstance(pred, torch.Tensor) or not pred.is_cuda:
            raise RuntimeError("predictions must be a tensor on a HIP device (evaluation has no CPU fallback)")
        if pred.dtype != self._map_dtype:
            raise RuntimeError("%s.update takes the %s map of get_output (got %s)" % (type(self).__name__, self._map_dtype, pred.dtype))
        B = pred.shape[0]
        per = 3 if self._kind == _lib.EVAL_NORMALS else 1
        if pred.dim() < 3 or pred[0].numel() % per:
            raise RuntimeError("unexpected map shape %s" % (tuple(pred.shape),))
        HW = pred[0].numel() // per
        self._accum(pred.reshape(B, -1).contiguous(), gt, _lib.EVAL_FROM_MAP, B, self._channels or 1, HW)

    def _host(self):
        """the accumulator on the host: ONE device-to-host copy (zeros before the first update)"""
        if self._acc is None:
            return torch.zeros(self._slots, dtype=torch.int64)
        return self._acc.cpu()

    def state(self):
        return self._unpack(self._host())

    def get_score(self, verbose=True, **kw):
        return self.score_from_state(self.state(), verbose, **kw)


def _jaccard_score(state, n, title, width, verbose, cat_names):
    """eval_semseg.py:88-107 / eval_human_parts.py:49-66"""
    tp, fp, fn = (state[k].tolist() for k in ('tp', 'fp', 'fn'))
    jac = [0] * n
    for i in range(n):
        jac[i] = float(tp[i]) / max(float(tp[i] + fp[i] + fn[i]), 1e-8)
    eval_result = dict()
    eval_result['mIoU'] = np.mean(jac) * 100
    if verbose:
        print('\n{0:s} mIoU: {1:.4f}\n'.format(title, eval_result['mIoU']))
        for i in range(n):
            name = str(cat_names[i]) if cat_names is not None else str(i)
            print('{0:s}{1:s}{2:.4f}'.format(name, ' ' * max(width - len(name), 0), 100 * jac[i]))
    return eval_result


class _ConfusionMeter(_Meter):
    _kind = _lib.EVAL_CONFUSION
    _map_dtype = torch.int64

    def _fields(self, device):
        return dict(n_classes=self.n_classes, ignore=float(self.ignore_idx))

    def _unpack(self, h):
        n = self.n_classes
        return dict(tp=h[:n].clone(), fp=h[n:2 * n].clone(), fn=h[2 * n:3 * n].clone())


class SemsegMeter(_ConfusionMeter):
    """eval_semseg.py:40-107: per-class tp / fp / fn over the valid pixels, mIoU.  A label outside [0, n_classes) that is not the ignore
    value counts as a false positive of the predicted class only."""
    _DATABASES = {'PASCALContext': (20, True), 'NYUD': (40, False), 'Cityscapes3D': (19, False)}

    def __init__(self, database, ignore_idx=255):
        if database not in self._DATABASES:
            raise NotImplementedError
        n_classes, has_bg = self._DATABASES[database]
        self.n_classes = n_classes + int(has_bg)
        self.ignore_idx = ignore_idx
        self._init_state(3 * self.n_classes)

    def score_from_state(self, state, verbose=True, cat_names=None):
        return _jaccard_score(state, self.n_classes, 'Semantic Segmentation', 20, verbose, cat_names)


class HumanPartsMeter(_ConfusionMeter):
    """eval_human_parts.py:20-66"""

    def __init__(self, database, ignore_idx=255):
        assert (database == 'PASCALContext')
        self.database = database
        self.n_parts = 6
        self.n_classes = self.n_parts + 1
        self.ignore_idx = ignore_idx
        self._init_state(3 * self.n_classes)

    def score_from_state(self, state, verbose=True, cat_names=None):
        return _jaccard_score(state, self.n_classes, 'Human Parts', 15, verbose, cat_names)


class SaliencyMeter(_Meter):
    """eval_sal.py:12-79: true / predicted / actual positives at every threshold of arange(step, 1, step), max F-score.  The device
    keeps a histogram over k = the number of thresholds a pixel's score reaches; predicted_positives[i] = sum of pp_hist[k] for k > i."""
    _kind = _lib.EVAL_SAL
    _channels = 2

    def __init__(self, ignore_index=255, threshold_step=None, beta_squared=1):
        self.ignore_index = ignore_index
        self.beta_squared = beta_squared
        self.thresholds = torch.arange(threshold_step, 1, threshold_step)
        th = self.thresholds.float()
        T = th.numel()
        if T < 1 or T > 255 or not bool((th[1:] > th[:-1]).all()):
            raise ValueError("thresholds must ascend and number 1 to 255")
        self._th_host = th
        self._init_state(2 * (T + 1) + 1)

    def update(self, preds, target):
        """preds: the [B, H, W] saliency map of get_output; target [B, 1, H, W] or [B, H, W]"""
        return super().update(preds, target)

    def _fields(self, device):
        th = self._extra.get(device)
        if th is None:
            th = self._extra[device] = self._th_host.to(device)      # the fp32 values torch.arange gave, never recomputed
        return dict(thresholds=th, n_thresh=th.numel(), ignore=float(self.ignore_index))

    def _unpack(self, h):
        T = self._th_host.numel()
        pp_hist, tp_hist, ap = h[:T + 1].clone(), h[T + 1:2 * (T + 1)].clone(), h[2 * (T + 1)].clone()
        above = lambda hist: (hist.sum() - torch.cumsum(hist, 0))[:T]          # noqa: E731   sum over k > i
        return dict(pp_hist=pp_hist, tp_hist=tp_hist, true_positives=above(tp_hist), predicted_positives=above(pp_hist),
                    actual_positives=ap.expand(T).clone())

    def score_from_state(self, state, verbose=False):
        true_positives, predicted_positives, actual_positives = (state[k].float() for k in
                                                                 ('true_positives', 'predicted_positives', 'actual_positives'))
        precision = true_positives.float() / predicted_positives
        recall = true_positives.float() / actual_positives
        num = (1 + self.beta_squared) * precision * recall
        denom = self.beta_squared * precision + recall
        fscore = num / denom
        fscore[fscore != fscore] = 0
        return {'maxF': fscore.max().item() * 100}

    def get_score(self, verbose=False):
        return self.score_from_state(self.state(), verbose)


class DepthMeter(_Meter):
    """eval_depth.py:19-71.  DepthMeter(max_depth, min_depth) evaluates min_depth < gt < max_depth (TaskPrompter);
    DepthMeter(ignore_index=255) evaluates gt != ignore_index (InvPT's DepthMeter, TaskPrompter's DepthMeter_legacy): pass it by keyword."""
    _kind = _lib.EVAL_DEPTH
    _channels = 1

    def __init__(self, max_depth=None, min_depth=None, *, ignore_index=None):
        if ignore_index is None and (max_depth is None or min_depth is None):
            raise ValueError("DepthMeter needs max_depth and min_depth, or ignore_index")
        self.max_depth, self.min_depth, self.ignore_index = max_depth, min_depth, ignore_index
        self._init_state(5)

    def _fields(self, device):
        if self.ignore_index is not None:
            return dict(mask_mode=1, ignore=float(self.ignore_index))
        return dict(mask_mode=0, max_depth=float(self.max_depth), min_depth=float(self.min_depth))

    def _unpack(self, h):
        f = h.view(torch.float64)
        return dict(n_valid=h[0].clone(), total_rmses=f[1].clone(), total_log_rmses=f[2].clone(), abs_rel=f[3].clone(), sq_rel=f[4].clone())

    def score_from_state(self, state, verbose=True):
        n_valid = float(state['n_valid'])
        total_rmses, total_log_rmses, abs_rel, sq_rel = (float(state[k]) for k in ('total_rmses', 'total_log_rmses', 'abs_rel', 'sq_rel'))
        eval_result = dict()
        eval_result['rmse'] = np.sqrt(total_rmses / n_valid)
        eval_result['log_rmse'] = np.sqrt(total_log_rmses / n_valid)
        eval_result['abs_rel'] = abs_rel / n_valid
        eval_result['sq_rel'] = sq_rel / n_valid
        if verbose:
            print('Results for depth prediction')
            for x in eval_result:
                print('{0:s}{1:s}{2:.4f}'.format(x, ' ' * (15 - len(x)), eval_result[x]))
        return eval_result


class NormalsMeter(_Meter):
    """eval_normals.py:27-51: mean angular error in degrees, through the reference's round trip map -> 2 map / 255 - 1 -> normalise."""
    _kind = _lib.EVAL_NORMALS
    _channels = 3
    _label_channels = 3

    def __init__(self, ignore_index=255):
        self.ignore_index = ignore_index
        self._init_state(2)

    def _fields(self, device):
        return dict(ignore=float(self.ignore_index))

    def _unpack(self, h):
        return dict(total=h[0].clone(), sum_deg_diff=h.view(torch.float64)[1].clone())

    def score_from_state(self, state, verbose=False):
        eval_result = dict()
        eval_result['mean'] = float(state['sum_deg_diff']) / int(state['total'])
        return eval_result

    def get_score(self, verbose=False):
        return self.score_from_state(self.state(), verbose)


class EdgeMeter(_Meter):
    """eval_edge.py:13-44 with loss_functions.py:56-88: the balanced BCE-with-logits of map / 255 over the valid pixels.  A batch of one
    is evaluated like any other (the reference raises IndexError there).  pos_weight=None, the HED-style weighting by label frequency, is
    not implemented (the reference's factory always passes p['edge_w'])."""
    _kind = _lib.EVAL_EDGE
    _channels = 1

    def __init__(self, pos_weight, ignore_index):
        if pos_weight is None:
            raise NotImplementedError("EdgeMeter(pos_weight=None): the HED-style weighting by label frequency is not implemented")
        self.pos_weight = pos_weight
        self.ignore_index = ignore_index
        self._init_state(2)

    def _fields(self, device):
        return dict(pos_weight=float(self.pos_weight), ignore=float(self.ignore_index))

    def _unpack(self, h):
        return dict(n=h[0].clone(), loss=h.view(torch.float64)[1].clone())

    def score_from_state(self, state, verbose=True):
        eval_dict = {'loss': float(state['loss']) / int(state['n'])}
        if verbose:
            print('\n Edge Detection Evaluation')
            print('Edge Detection Loss %.3f' % (eval_dict['loss']))
        return eval_dict


def get_single_task_meter(p, database, task):
    """evaluate_utils.py:35-66"""
    if task == 'semseg':
        return SemsegMeter(database, ignore_idx=p.ignore_index)
    elif task == 'human_parts':
        return HumanPartsMeter(database, ignore_idx=p.ignore_index)
    elif task == 'normals':
        return NormalsMeter(ignore_index=p.ignore_index)
    elif task == 'sal':
        return SaliencyMeter(ignore_index=p.ignore_index, threshold_step=0.05, beta_squared=0.3)
    elif task == 'depth':
        return DepthMeter(max_depth=p.TASKS.depth_max, min_depth=p.TASKS.depth_min)
    elif task == 'edge':
        return EdgeMeter(pos_weight=p['edge_w'], ignore_index=p.ignore_index)
    else:
        raise NotImplementedError


class PerformanceMeter(object):
    """evaluate_utils.py:13-33: one meter per task.  update / update_from_logits launch kernels only (no host synchronisation)."""

    def __init__(self, p, tasks):
        self.database = p['train_db_name']
        self.tasks = tasks
        self.meters = {t: get_single_task_meter(p, self.database, t) for t in self.tasks}

    def to(self, device):
        for t in self.tasks:
            self.meters[t].to(device)
        return self

    def reset(self):
        for t in self.tasks:
            self.meters[t].reset()

    def update(self, pred, gt):
        for t in self.tasks:
            self.meters[t].update(pred[t], gt[t])

    def update_from_logits(self, output, gt):
        for t in self.tasks:
            self.meters[t].update_from_logits(output[t], gt[t])

    def get_score(self, verbose=True):
        eval_dict = {}
        for t in self.tasks:
            eval_dict[t] = self.meters[t].get_score(verbose)
        return eval_dict
