"""ControlledUnetModel with IP-Adapter cross-attentions (API of the reference's cldm/cldm_style.py:22-45).

The residual injection is cldm.cldm's; `context` is the reference's per-block list of [txt, ip] pairs
(cldm_ctrlora_style_inference.py:184-188), or a plain text tensor.
"""
from cldm.cldm import ControlNet  # noqa: F401  (the style config's control_stage_config is the plain ControlNet family)
from ldm.modules.diffusionmodules.openaimodel_ip import UNetModel


def split_context(context):
    """[[txt, ip]] / [txt, ip] / txt -> (txt, ip or None)."""
    if isinstance(context, (list, tuple)):
        if len(context) == 1 and isinstance(context[0], (list, tuple)):
            context = context[0]
        txt, ip = context
        return txt, ip
    return context, None


class ControlledUnetModel(UNetModel):
    def forward(self, x, timesteps=None, context=None, control=None, only_mid_control=False, **kwargs):
        from ctrlora_amd.engine import CtrLoRAEngine
        txt, ip = split_context(context)
        eng = CtrLoRAEngine.from_executors(self.executor(), [])
        return eng.forward_external_control(x, timesteps, txt, control, only_mid_control, context_ip=ip)
