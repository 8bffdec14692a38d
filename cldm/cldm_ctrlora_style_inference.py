"""CtrLoRA inference with IP-Adapter style control (API of the reference's cldm/cldm_ctrlora_style_inference.py).

ControlNetInference is the non-style class: it has no image-prompt weights and sees the text context only.
ControlInferenceLDM.apply_model (:156-189) takes `c_ip` from conds[0] and hands it to the UNet's IPCrossAttention
layers only; a conditioning without `c_ip` (or with every ip_scale at 0) is exactly the plain multi-LoRA inference.
"""
import torch

from cldm.cldm_ctrlora_inference import ControlInferenceLDM as _PlainInferenceLDM
from cldm.cldm_ctrlora_inference import ControlNetInference  # noqa: F401


class ControlInferenceLDM(_PlainInferenceLDM):
    @torch.no_grad()
    def apply_model(self, x_noisy, t, conds, *args, **kwargs):
        if isinstance(conds, dict):
            conds = [conds]
        assert isinstance(conds, (list, tuple))
        assert len(conds) == self.control_model.lora_num
        assert len(self.lora_weights) == self.control_model.lora_num
        cond_txt = torch.cat(conds[0]["c_crossattn"], 1)
        cond_ip = torch.cat(conds[0]["c_ip"], 1) if conds[0].get("c_ip") is not None else None
        hints = None
        if conds[0]["c_concat"][0] is not None:
            hints = [self._hint_latent(c) for c in conds]
        return self._run(x_noisy, t, cond_txt, hints, weights=list(self.lora_weights), context_ip=cond_ip)
