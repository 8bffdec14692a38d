"""High-level inference API (same surface as the reference's api.py:15-163).

    from api import CtrLoRA
    ctrlora = CtrLoRA(num_loras=1)
    ctrlora.create_model(sd_file=..., basecn_file=..., lora_files=(...,))
    images = ctrlora.sample(cond_image_paths=..., prompt=..., n_prompt=..., num_samples=..., ddim_steps=..., scale=...)
    # start from an image (img2img: the last int(strength * ddim_steps) steps from the noised image) ...
    images = ctrlora.sample(..., init_image="photo.png", strength=0.6)
    # ... or repaint the marked pixels of it and keep the rest (with the inpainting / outpainting / blur / grayscale LoRAs)
    images = ctrlora.sample(..., init_image="photo.png", mask_image=marked_u8)

`create_model` assembles the inference model from three kinds of checkpoint: SD1.5 (UNet, VAE, CLIP), the Base
ControlNet (everything under `control_model.` that is NOT LoRA-file material) and one LoRA file per slot
(`check_key` material: LoRA layers, zero convs, norm layers), each loaded into its switchable bank with the
reference's sequence switch_lora(i) -> load_state_dict(strict=False) -> copy_weights_to_switchable().
The denoising loop runs on the MI355X engine (cldm.ddim_hacked.DDIMSampler -> ControlInferenceLDM.apply_model).
"""
import os

import numpy as np
import torch

from cldm.ddim_hacked import DDIMSampler
from cldm.model import create_model, load_state_dict

_HERE = os.path.dirname(os.path.abspath(__file__))


def hwc3(x: np.ndarray) -> np.ndarray:
    """uint8 image -> H x W x 3 (grey replicated; RGBA composited on white), as annotator/util.py:11-27."""
    assert x.dtype == np.uint8
    if x.ndim == 2:
        x = x[:, :, None]
    assert x.ndim == 3 and x.shape[2] in (1, 3, 4)
    if x.shape[2] == 3:
        return x
    if x.shape[2] == 1:
        return np.repeat(x, 3, axis=2)
    rgb, a = x[:, :, :3].astype(np.float32), x[:, :, 3:4].astype(np.float32) / 255.0
    return (rgb * a + 255.0 * (1.0 - a)).clip(0, 255).astype(np.uint8)


def center_crop_to_common(a: np.ndarray, b: np.ndarray):
    """Crop two H x W x C images around their centres to the smaller height and the smaller width (api.py:113-126)."""
    def crop(img, H, W):
        h, w = img.shape[:2]
        if h > H:
            img = img[(h - H) // 2:(h + H) // 2]
        if w > W:
            img = img[:, (w - W) // 2:(w + W) // 2]
        return img
    H, W = min(a.shape[0], b.shape[0]), min(a.shape[1], b.shape[1])
    a, b = crop(a, H, W), crop(b, H, W)
    assert a.shape[:2] == b.shape[:2]
    return a, b


def load_image(image) -> np.ndarray:
    """A path, a PIL image or a uint8 array -> uint8 H x W x 3."""
    if isinstance(image, (str, os.PathLike)):
        from PIL import Image
        image = Image.open(image)
    return hwc3(np.asarray(image))


def center_crop_to(img: np.ndarray, H: int, W: int) -> np.ndarray:
    """Crop an H' x W' [x C] image around its centre to H x W; an image smaller than that is refused."""
    h, w = img.shape[:2]
    if h < H or w < W:
        raise ValueError(f"image {h} x {w} is smaller than the condition image {H} x {W}")
    return img[(h - H) // 2:(h - H) // 2 + H, (w - W) // 2:(w - W) // 2 + W]


def img2img_steps(strength: float, ddim_steps: int) -> int:
    """How many of the schedule's steps an img2img run takes: t_enc = min(int(strength * ddim_steps), ddim_steps - 1)."""
    t_enc = min(int(strength * ddim_steps), ddim_steps - 1)
    if t_enc <= 0:
        raise ValueError(f"strength {strength} of {ddim_steps} steps leaves no step to run")
    return t_enc


def latent_keep_mask(mask_image: np.ndarray, h: int, w: int) -> torch.Tensor:
    """uint8 H x W, non-zero = repaint  ->  fp32 (1, 1, h, w) with 1 = KEEP (the convention of DDIMSampler.sample(mask=)): an
    8 x 8 cell of pixels is one latent position, kept only if none of its pixels is marked."""
    mk = np.asarray(mask_image)
    if mk.ndim != 2 or mk.dtype != np.uint8:
        raise ValueError("mask_image is a uint8 H x W array (non-zero = repaint)")
    if mk.shape != (8 * h, 8 * w):
        raise ValueError(f"mask_image {mk.shape} does not cover the {h} x {w} latent ({8 * h} x {8 * w} pixels)")
    marked = (mk != 0).reshape(h, 8, w, 8).any(axis=(1, 3))
    return torch.from_numpy(~marked).float().reshape(1, 1, h, w)


def check_edit_args(init_image, strength, mask_image):
    """The argument rules of the image-editing modes; returns 'plain', 'img2img' or 'masked'."""
    if not 0.0 < strength <= 1.0:
        raise ValueError(f"strength {strength} is outside (0, 1]")
    if mask_image is not None:
        if init_image is None:
            raise ValueError("mask_image needs init_image: the pixels that are kept come from it")
        if strength < 1.0:
            raise ValueError("mask_image with strength < 1: the sampler's decode() has no mask (run the full schedule)")
        return "masked"
    if strength < 1.0:
        if init_image is None:
            raise ValueError("strength < 1 needs init_image")
        return "img2img"
    return "plain"


@torch.no_grad()
def encode_init(model, image: np.ndarray, num_samples: int) -> torch.Tensor:
    """uint8 H x W x 3 -> the first-stage latent z0 [num_samples, 4, H / 8, W / 8] (one posterior draw per sample)."""
    x = torch.from_numpy(image.copy()).float().to(model.device) / 127.5 - 1.0
    x = x.permute(2, 0, 1).unsqueeze(0).repeat(num_samples, 1, 1, 1).contiguous()
    return model.get_first_stage_encoding(model.encode_first_stage(x)).float()


@torch.no_grad()
def img2img_latents(sampler, z0, cond, uncond, ddim_steps, strength, scale, eta=0.):
    """The reference's img2img on DDIMSampler: noise z0 to step t_enc of the schedule (stochastic_encode), then the last t_enc
    steps from there (decode)."""
    t_enc = img2img_steps(strength, ddim_steps)
    sampler.make_schedule(ddim_num_steps=ddim_steps, ddim_eta=eta, verbose=False)
    z = sampler.stochastic_encode(z0, torch.full((z0.shape[0],), t_enc, device=z0.device, dtype=torch.long))
    return sampler.decode(z, cond, t_enc, unconditional_guidance_scale=scale, unconditional_conditioning=uncond)


class CtrLoRA:
    def __init__(self, num_loras=1):
        self.model = None
        self.num_loras = num_loras
        if num_loras not in (1, 2):
            raise ValueError("Invalid number of LoRAs. Only 1 or 2 are supported.")
        name = "ctrlora_sd15_rank128_1lora.yaml" if num_loras == 1 else "ctrlora_sd15_rank128_2loras.yaml"
        self.config_file = os.path.join("configs", "inference", name)

    @staticmethod
    def check_key(k):
        return "lora_layer" in k or "zero_convs" in k or "middle_block_out" in k or "norm" in k

    # ------------------------------------------------------------------ checkpoint assembly
    def load_weights(self, model, sd_state_dict=None, cn_state_dict=None, lora_state_dicts=()):
        """The load sequence of create_model on already-read state dicts (api.py:46-62)."""
        if sd_state_dict is not None:
            model.load_state_dict(sd_state_dict, strict=False)
        if cn_state_dict is not None:
            base = {k: v for k, v in cn_state_dict.items() if k.startswith("control_model") and not self.check_key(k)}
            model.load_state_dict(base, strict=False)
        for i, lora_sd in enumerate(lora_state_dicts):
            lora = {k: v for k, v in lora_sd.items() if self.check_key(k)}
            model.control_model.switch_lora(i)
            model.load_state_dict(lora, strict=False)
            model.control_model.copy_weights_to_switchable()
        return model

    def create_model(self, sd_file="ckpts/sd15/v1-5-pruned.ckpt",
                     basecn_file="ckpts/ctrlora-basecn/ctrlora_sd15_basecn700k.ckpt",
                     lora_files=("ckpts/ctrlora-loras/novel-conditions/"
                                 "ctrlora_sd15_basecn700k_lineart_rank128_1kimgs_1ksteps.ckpt",)):
        if not isinstance(lora_files, (tuple, list)):
            lora_files = (lora_files,)
        for f in (sd_file, basecn_file, *lora_files):
            assert os.path.exists(f), f"File not found: {f}"
        cfg = self.config_file if os.path.exists(self.config_file) else os.path.join(_HERE, self.config_file)
        self.model = create_model(cfg).cuda()
        self.load_weights(self.model, sd_state_dict=load_state_dict(sd_file, location="cpu"))
        self.load_weights(self.model, cn_state_dict=load_state_dict(basecn_file, location="cpu"))
        self.load_weights(self.model, lora_state_dicts=[load_state_dict(f, location="cpu") for f in lora_files])

    # ------------------------------------------------------------------ sampling
    def sample(self, cond_image_paths, prompt, n_prompt="", num_samples=1, ddim_steps=20, scale=7.5,
               lora_weights=(1.0, 1.0), init_image=None, strength=1.0, mask_image=None, composite=True):
        """init_image (a path, a PIL image or a uint8 H x W [x C] array, centre-cropped to the condition image) with
        0 < strength < 1: img2img.  With mask_image (uint8 H x W of the condition image's size, non-zero = repaint): the full
        schedule with the unmarked latent cells re-noised from init_image at every step; composite: the unmarked PIXELS of the
        result are init_image's own."""
        from PIL import Image
        assert self.model is not None, "Model is not loaded. Please call create_model() first."
        if not isinstance(cond_image_paths, (tuple, list)):
            cond_image_paths = (cond_image_paths,)
        assert len(cond_image_paths) == self.num_loras, f"Expected {self.num_loras} images, got {len(cond_image_paths)}"
        images = [hwc3(np.array(Image.open(p))) for p in cond_image_paths]
        if self.num_loras == 1:
            return self.sample_1lora(images[0], prompt, n_prompt, num_samples, ddim_steps, scale, init_image=init_image,
                                     strength=strength, mask_image=mask_image, composite=composite)
        return self.sample_2loras(images, prompt, n_prompt, num_samples, ddim_steps, scale, lora_weights, init_image=init_image,
                                  strength=strength, mask_image=mask_image, composite=composite)

    def _control(self, image: np.ndarray, num_samples: int) -> torch.Tensor:
        c = torch.from_numpy(image.copy()).float().cuda() / 255.0           # H x W x 3 in [0, 1]
        return c.permute(2, 0, 1).unsqueeze(0).repeat(num_samples, 1, 1, 1).contiguous()

    @torch.no_grad()
    def _run(self, images, prompt, n_prompt, num_samples, ddim_steps, scale, lora_weights=None, init_image=None, strength=1.0,
             mask_image=None, composite=True):
        from PIL import Image
        H, W, _ = images[0].shape
        m = self.model
        mode = check_edit_args(init_image, strength, mask_image)
        if mode != "plain":
            init = center_crop_to(load_image(init_image), H, W)
        if mode == "masked":
            if np.asarray(mask_image).ndim != 2:
                raise ValueError("mask_image is a uint8 H x W array (non-zero = repaint)")
            marked = center_crop_to(np.asarray(mask_image), H, W)
            keep = latent_keep_mask(marked, H // 8, W // 8).to(m.device)
        elif mode == "img2img":
            img2img_steps(strength, ddim_steps)          # refuse before any model work
        txt = m.get_learned_conditioning([prompt] * num_samples)
        ntxt = m.get_learned_conditioning([n_prompt] * num_samples)
        conds = [{"c_concat": [self._control(im, num_samples)], "c_crossattn": [txt]} for im in images]
        unconds = [{"c_concat": c["c_concat"], "c_crossattn": [ntxt]} for c in conds]
        m.control_scales = [1] * 13
        if lora_weights is not None:
            m.lora_weights = [lora_weights[0], lora_weights[1]]
        single = len(images) == 1
        cond, uncond = (conds[0], unconds[0]) if single else (conds, unconds)
        if mode == "img2img":
            samples = img2img_latents(DDIMSampler(m), encode_init(m, init, num_samples), cond, uncond, ddim_steps, strength, scale)
        else:
            edit = dict(mask=keep, x0=encode_init(m, init, num_samples)) if mode == "masked" else {}
            samples, _ = DDIMSampler(m).sample(
                ddim_steps, num_samples, (4, H // 8, W // 8), cond, verbose=False, eta=0,
                unconditional_guidance_scale=scale, unconditional_conditioning=uncond, **edit)
        x = m.decode_first_stage(samples)
        x = (x.permute(0, 2, 3, 1) * 127.5 + 127.5).cpu().numpy().clip(0, 255).astype(np.uint8)
        if mode == "masked" and composite:
            x[:, marked == 0] = init[marked == 0]
        return [Image.fromarray(x[i]) for i in range(num_samples)]

    def sample_1lora(self, detected_image, prompt, n_prompt="", num_samples=1, ddim_steps=20, scale=7.5, init_image=None,
                     strength=1.0, mask_image=None, composite=True):
        return self._run([detected_image], prompt, n_prompt, num_samples, ddim_steps, scale, init_image=init_image,
                         strength=strength, mask_image=mask_image, composite=composite)

    def sample_2loras(self, detected_images, prompt, n_prompt="", num_samples=1, ddim_steps=20, scale=7.5,
                      lora_weights=(1.0, 1.0), init_image=None, strength=1.0, mask_image=None, composite=True):
        a, b = center_crop_to_common(*detected_images)
        return self._run([a, b], prompt, n_prompt, num_samples, ddim_steps, scale, lora_weights, init_image=init_image,
                         strength=strength, mask_image=mask_image, composite=composite)
