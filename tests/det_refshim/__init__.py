"""Import stand-ins that let the reference's detection_toolbox/det_head.py and fpn.py import and run on CPU (test fixtures only).

mmcv 1.6.2 and termcolor are not dependencies of this project.  The layers the head builds through mmcv are restated here in plain torch:
ConvModule (conv -> norm -> act), ModulatedDeformConv2dPack (tests/det_ref.dcn_v2), BaseModule, Registry, auto_fp16; termcolor.colored is the
identity.  Put this directory on sys.path (before the reference's TaskPrompter root) to use them."""
