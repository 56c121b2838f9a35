"""multi-task-transformer_amd — MI355X (gfx950) native hot path of prismformore/Multi-Task-Transformer.

The directory name carries a hyphen (it mirrors the reference repository's name), so import it through
`importlib.import_module("multi-task-transformer_amd")` or the `mtt_amd` alias module at the repo root.
"""
from . import _lib, ops, autograd_path, factory, losses, det_losses, det_head, det_decode, det_model, optim, checkpoints, iou3d, taskprompter_swin, graphs, evaluation, augment, cs3d, render  # noqa: F401
from .taskprompter import (ConvHead, DEConvHead, TaskPrompter, TaskPrompterWrapper,  # noqa: F401
                           taskprompter_vit_base_patch16_384, taskprompter_vit_large_patch16_384)
from .invpt import (MLPHead, TransformerDecoder, TransformerNet, VisionTransformer, vit_large_patch16_384)  # noqa: F401,E402
from .taskprompter_swin import TaskPrompterSwin, taskprompter_swin_base_patch4_window12_384  # noqa: F401,E402
from .evaluation import (get_output, PerformanceMeter, SemsegMeter, HumanPartsMeter, NormalsMeter, SaliencyMeter, DepthMeter, EdgeMeter)  # noqa: F401,E402
from .augment import DeviceAugment, AugParams  # noqa: F401,E402
from .cs3d import Cityscapes3DPrepare  # noqa: F401,E402
from .render import PredictionRenderer, vis_pred_for_one_task, save_model_pred_for_one_task  # noqa: F401,E402
