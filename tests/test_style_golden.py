"""IP-Adapter style control against the reference, no GPU (fixture: tests/golden/make_golden_style.py).

  * the mirror's tiny style UNet has the reference's state-dict keys / shapes and IPCrossAttention order;
  * configs/inference/ctrlora_style_sd15_rank128_1lora.yaml builds the style LDM through instantiate_from_config;
  * cldm.style_helpers maps IP-Adapter checkpoints and sets the ip_scale targets as the app's change_key /
    load_state_dict_ip do; ImageProjModel is Linear -> 4 tokens -> LayerNorm.
"""
import os

import pytest
import torch
import yaml

from tests.util import GOLDEN, ROOT

PREFIX = "model.diffusion_model."


def _gold():
    return torch.load(os.path.join(GOLDEN, "style_tiny.pt"), weights_only=False)


def _tiny_style_ldm():
    from ldm.util import instantiate_from_config
    with open(os.path.join(ROOT, "configs", "inference", "ctrlora_style_sd15_rank128_1lora.yaml")) as f:
        cfg = yaml.safe_load(f)["model"]
    p = cfg["params"]
    for k in ("control_stage_config", "unet_config"):
        p[k]["params"].update(model_channels=64, context_dim=96)
    p["control_stage_config"]["params"]["lora_rank"] = 32
    p["first_stage_config"] = {"target": "torch.nn.Identity"}
    p["cond_stage_config"] = {"target": "torch.nn.Identity"}
    return instantiate_from_config(cfg)


def test_style_yaml_builds_and_unet_keys_match_reference():
    g = _gold()
    model = _tiny_style_ldm()
    assert type(model).__module__ == "cldm.cldm_ctrlora_style_inference"
    assert type(model.control_model).__name__ == "ControlNetInference"
    unet = model.model.diffusion_model
    assert type(unet).__module__ == "cldm.cldm_style"
    assert {k: list(v.shape) for k, v in unet.state_dict().items()} == g["unet_keys"]
    from ldm.modules.attention_ip import IPCrossAttention
    assert [n for n, m in unet.named_modules() if isinstance(m, IPCrossAttention)] == g["ip_layers"]
    assert all(float(v) == 0.0 for k, v in unet.state_dict().items() if k.endswith("ip_scale"))


def test_key_mapping_matches_the_app():
    from cldm.style_helpers import ip_adapter_state, ip_layer_names
    from cldm.cldm_style import ControlledUnetModel
    from tests.test_style_mirror import UNET_SD15
    app = _gold()["app"]
    with torch.device("meta"):
        unet = ControlledUnetModel(**UNET_SD15)
    names = ip_layer_names(unet)
    assert len(names) == 16
    ckpt = {k: torch.tensor(v) for k, v in app["ckpt"].items()}
    mapped = {k: float(v) for k, v in ip_adapter_state(ckpt, names).items()}
    assert mapped == app["change_key"]


@pytest.mark.parametrize("target", ["Load original IP-Adapter", "Load only style blocks", "Load style+layout block"])
def test_ip_scale_targets_match_the_app(target):
    from cldm.style_helpers import ip_scale_state
    st = ip_scale_state(target, 0.75)
    assert sorted(st) == _gold()["app"]["scale_keys"][target]
    assert all(float(v) == 0.75 for v in st.values())


def test_image_proj_model():
    from cldm.style_helpers import ImageProjModel
    torch.manual_seed(0)
    m = ImageProjModel()
    e = torch.randn(3, 1024)
    y = m(e)
    assert y.shape == (3, 4, 768)
    want = torch.nn.functional.layer_norm((e @ m.proj.weight.t() + m.proj.bias).reshape(3, 4, 768), (768,),
                                          m.norm.weight, m.norm.bias)
    assert torch.allclose(y, want, atol=1e-5)
    assert sorted(m.state_dict()) == ["norm.bias", "norm.weight", "proj.bias", "proj.weight"]
