"""IP-Adapter style control: the class API (no GPU).

The reference's style UNet (ldm/modules/diffusionmodules/openaimodel_ip.py, ldm/modules/attention_ip.py:196-289,
422-520) differs from the plain one by `to_k_ip`, `to_v_ip` (bias-free) and an `ip_scale` buffer in `attn2` of every
transformer block; `attn1` stays plain.  The mirror must build that tree so IP-Adapter state dicts load unchanged.
"""
import torch

UNET_SD15 = dict(image_size=32, in_channels=4, out_channels=4, model_channels=320, attention_resolutions=[4, 2, 1],
                 num_res_blocks=2, channel_mult=[1, 2, 4, 4], num_heads=8, use_spatial_transformer=True,
                 transformer_depth=1, context_dim=768, use_checkpoint=True, legacy=False)


def test_style_unet_state_dict_keys():
    from cldm import cldm_style
    from ldm.modules.diffusionmodules.openaimodel import UNetModel as PlainUNet
    with torch.device("meta"):
        style = cldm_style.ControlledUnetModel(**UNET_SD15)
        plain = PlainUNet(**UNET_SD15)
    ks, kp = list(style.state_dict().keys()), list(plain.state_dict().keys())
    extra = [k for k in ks if k not in set(kp)]
    assert set(kp) <= set(ks)
    attn2 = sorted({k.split(".attn2.")[0] + ".attn2" for k in extra})
    assert len(attn2) == 16 and all(n.endswith(".attn2") for n in attn2)
    assert sorted(extra) == sorted(f"{n}.{s}" for n in attn2 for s in ("to_k_ip.weight", "to_v_ip.weight", "ip_scale"))
    # module order: input_blocks 1, 2, 4, 5, 7, 8, the middle block, output_blocks 3-11 (the IP-Adapter processor order)
    blocks = [n.split(".transformer_blocks")[0] for n in attn2]
    order = [n for n, m in style.named_modules() if n.endswith(".attn2")]
    assert [o.split(".transformer_blocks")[0] for o in order] == [
        "input_blocks.1.1", "input_blocks.2.1", "input_blocks.4.1", "input_blocks.5.1", "input_blocks.7.1",
        "input_blocks.8.1", "middle_block.1"] + [f"output_blocks.{i}.1" for i in range(3, 12)]
    assert sorted(blocks) == sorted(o.split(".transformer_blocks")[0] for o in order)


def test_split_context():
    from cldm.cldm_style import split_context
    a, b = torch.zeros(1), torch.ones(1)
    assert split_context([[a, b]]) == (a, b)
    assert split_context([a, None]) == (a, None)
    assert split_context(a) == (a, None)


def test_style_inference_ldm_is_the_plain_one_plus_c_ip():
    from cldm import cldm_ctrlora_inference as plain, cldm_ctrlora_style_inference as style
    assert style.ControlNetInference is plain.ControlNetInference
    assert issubclass(style.ControlInferenceLDM, plain.ControlInferenceLDM)
