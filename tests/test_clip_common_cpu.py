"""What the two CLIP towers share (ctrlora_amd/engine/clip_common.py), on the CPU with the recording stand-in of
tests/test_engine_launch_sequence.py in place of libctrlora_hip.so: the address rule of the executors' load(), and ExecutorHost --
the mixin of CLIPVisionEncoder, CLIPTextEncoder and FrozenCLIPEmbedder -- over a stub executor class.  No kernel is launched."""
import warnings

import pytest
import torch

from ctrlora_amd import hip
from ctrlora_amd.engine import clip_text, vit
from tests.test_clip_text_cpu import TINY as TEXT_TINY, hf_text_model
from tests.test_clip_vision_cpu import TINY as VISION_TINY, hf_model
from tests.test_engine_launch_sequence import Recorder

DTYPES = [torch.bfloat16, torch.float32]


@pytest.fixture
def no_library(monkeypatch):
    monkeypatch.setattr(hip, "_lib", Recorder({}))


def clone(sd):
    return {k: v.clone() for k, v in sd.items()}          # (an fp32 executor on the CPU may alias what it is given)


def tensors(w):
    out = {k: t for k, t in w.items() if k != "layers"}
    out.update({f"layers[{i}].{k}": t for i, lay in enumerate(w["layers"]) for k, t in lay.items()})
    return out


def check_load_keeps_addresses(make, sd1, sd2):
    ex = make(clone(sd1))
    before = {k: (t.data_ptr(), t.dtype, t.clone()) for k, t in tensors(ex.w).items()}
    ex.load(clone(sd2))
    fresh = tensors(make(clone(sd2)).w)                    # what a new executor packs from the second state dict
    after = tensors(ex.w)
    assert list(after) == list(before) == list(fresh) and len(after) > 12
    for k, t in after.items():
        assert (t.data_ptr(), t.dtype) == before[k][:2], k
        assert torch.equal(t, fresh[k]) and not torch.equal(t, before[k][2]), k
    return ex


@pytest.mark.parametrize("dtype", DTYPES)
def test_vision_load_refreshes_every_packed_tensor_in_place(dtype, no_library):
    make = lambda sd: vit.ClipVisionE(sd, VISION_TINY, dtype, "cpu")
    check_load_keeps_addresses(make, hf_model(VISION_TINY, seed=0).state_dict(), hf_model(VISION_TINY, seed=5).state_dict())


@pytest.mark.parametrize("dtype", DTYPES)
def test_text_load_refreshes_every_packed_tensor_in_place(dtype, no_library):
    make = lambda sd: clip_text.ClipTextE(sd, TEXT_TINY, dtype, "cpu")
    sd1, sd2 = hf_text_model(TEXT_TINY, seed=0).state_dict(), hf_text_model(TEXT_TINY, seed=5).state_dict()
    ex = check_load_keeps_addresses(make, sd1, sd2)
    assert "proj_w" in ex.w
    without = {k: v for k, v in clone(sd1).items() if k != "text_projection.weight"}
    with pytest.raises(ValueError, match="text_projection"):
        ex.load(without)
    plain = make(without)
    assert "proj_w" not in plain.w
    with pytest.raises(ValueError, match="text_projection"):
        plain.load(clone(sd1))
    plain.load({k: v for k, v in clone(sd2).items() if k != "text_projection.weight"})
    assert torch.equal(plain.w["tok"], ex.w["tok"])


# --------------------------------------------------------------------------- ExecutorHost

class StubExecutor:
    def __init__(self, state_dict, config, dtype, device):
        self.keys, self.config, self.dtype, self.device, self.loads = list(state_dict), config, dtype, torch.device(device), []

    def load(self, state_dict):
        self.loads.append(list(state_dict))


def vision_encoder():
    from cldm.style_helpers import CLIPVisionEncoder
    enc = CLIPVisionEncoder(VISION_TINY)
    return enc, enc, "_vit", None


def text_encoder():
    from cldm.style_helpers import CLIPTextEncoder
    enc = CLIPTextEncoder(TEXT_TINY)
    return enc, enc, "_txt", None


def frozen_embedder():
    from ldm.modules.encoders.modules import FrozenCLIPEmbedder
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        enc = FrozenCLIPEmbedder(version="no-such-local-model", device="cpu")
    return enc, enc.transformer, "_txt", torch.float32


@pytest.mark.parametrize("build", [vision_encoder, text_encoder, frozen_embedder])
def test_executor_host(build, monkeypatch):
    """(wrapper, the module that feeds the executor, the __dict__ slot, the default engine dtype: None follows the environment)"""
    enc, source, slot, default = build()
    monkeypatch.setattr(type(enc), "ENGINE_CLASS", StubExecutor)
    monkeypatch.delenv("CTRLORA_ENGINE_DTYPE", raising=False)
    assert type(enc).ENGINE_SLOT == slot and slot not in enc.__dict__ and enc.engine_dtype == default and enc.use_engine
    keys = list(enc.state_dict())
    ex = enc.engine()
    # built once from the source module, kept out of the children and the state dict
    assert enc.__dict__[slot] is ex and enc.engine() is ex
    assert ex.keys == list(source.state_dict()) and ex.config is source.config and ex.device == torch.device("cpu")
    assert list(enc.state_dict()) == keys and all(m is not ex for m in enc.modules()) and slot not in enc._modules
    # the dtype: what was set, else the wrapper's default, else the environment, else bf16
    assert ex.dtype == (default or torch.bfloat16)
    for env, want in (("fp32", torch.float32), ("F32", torch.float32), ("float32", torch.float32), ("bf16", torch.bfloat16)):
        monkeypatch.setenv("CTRLORA_ENGINE_DTYPE", env)
        enc.invalidate_engine()
        assert slot not in enc.__dict__ and enc.engine().dtype == (default or want), env
    for dtype in (torch.bfloat16, torch.float32):
        enc.set_engine_dtype(dtype)
        assert slot not in enc.__dict__, "set_engine_dtype keeps the old executor"
        assert enc.engine().dtype == dtype and enc.engine_dtype == dtype
    # load_state_dict on a live executor refreshes it in place: the same object, load() once, with the source's state dict
    ex = enc.engine()
    enc.load_state_dict(enc.state_dict())
    assert enc.__dict__[slot] is ex and ex.loads == [list(source.state_dict())]
    # ... unless the parameters are no longer where the executor is
    ex.device = torch.device("meta")
    enc.load_state_dict(enc.state_dict())
    assert slot not in enc.__dict__ and len(ex.loads) == 1
    # .to() / .float() / .cuda() go through _apply: the packed copies follow the parameters
    ex = enc.engine()
    enc.float()
    assert slot not in enc.__dict__ and enc.engine() is not ex
