"""PLMS sampler (API of the reference's ldm/models/diffusion/plms.py: PLMSSampler.make_schedule, sample, plms_sampling,
p_sample_plms; the method is Liu et al., "Pseudo Numerical Methods for Diffusion Models on Manifolds", arXiv:2202.09778).

The schedule is DDIM's with eta = 0.  Iteration i (table row S-1-i, time t_i) evaluates the guided e = eps(x, t_i) and forms
    i = 0:  x~ = upd(x, e).x_prev,  e_n = eps(x~, t_1),  e' = (e + e_n) / 2          (pseudo improved Euler, two evaluations)
    i = 1:  e' = (3 e - o1) / 2
    i = 2:  e' = (23 e - 16 o1 + 5 o2) / 12
    i >= 3: e' = (55 e - 59 o1 + 37 o2 - 9 o3) / 24                                   (Adams-Bashforth over the last e)
    x, pred_x0 = upd(x, e'):  pred_x0 = (x - sqrt(1-a_t) e') / sqrt(a_t),  x_prev = sqrt(a_prev) pred_x0 + sqrt(1 - a_prev) e'
where o1, o2, o3 are the e of the previous iterations (iteration 0's own e, not e_n).

What changes underneath, not in the results:
  * guidance + history write + Adams-Bashforth sum + update are one fused HIP kernel per model evaluation (cl_plms_step) on
    DDIM's [S][4] device table and a [4][n] ring of guided eps;
  * classifier-free guidance is one batch of 2B ordered [unconditional; conditional] as the reference batches it, for tensors
    AND for same-structure dict conditionings (the reference's torch.cat would raise on ControlLDM's dicts); other structures
    run as two passes of B;
  * with an engine model and S >= 4, iteration 0 (two evaluations) runs eagerly, and from iteration 1 on the iteration number
    and the model time live on the device: one step (cl_ddim_set_t, apply_model, cl_plms_step_dev, cl_tick) is captured as a
    hipGraph and replayed.  The order of a replayed step is derived from the device cursor, so one capture serves the second-,
    third- and fourth-order steps: 4 Python-level model calls however large S is.
Tensors outside the engine (CPU) take the same table through a plain-torch update in the reference's fp32 forms.

eta is always 0 (anything else raises, as in the reference), so the reference's sigma_t * noise term is identically zero:
`temperature` and `noise_dropout` are accepted and cannot act, and no randn is drawn for that term -- only the position of the
global RNG after a run differs from the reference.  ddim_use_original_steps, quantize_denoised, score_corrector,
dynamic_threshold and a non-eps parameterisation raise NotImplementedError, as in DDIMSampler here.
"""
import numpy as np
import torch

from ldm.models.diffusion.guided_loop import UNCOND_FIRST, batch_conds, context_kv, engine_of, guided_eps, hint_scope, run_steps
from ldm.modules.diffusionmodules.util import make_ddim_sampling_parameters, make_ddim_timesteps


def _combine(e, old):
    """e' of a multistep iteration from its own e and the earlier ones (oldest first), fp32: multiply, then ONE division."""
    if len(old) == 1:
        return (3 * e - old[-1]) / 2
    if len(old) == 2:
        return (23 * e - 16 * old[-1] + 5 * old[-2]) / 12
    return (55 * e - 59 * old[-1] + 37 * old[-2] - 9 * old[-3]) / 24


def _update(x, e, row):
    """upd(x, e') on one fp32 table row {a_t, a_prev, sigma_t, sqrt(1 - a_t)}, plain torch."""
    a_t, a_prev, sigma, s1m = row[0], row[1], row[2], row[3]
    pred_x0 = (x - s1m * e) / a_t.sqrt()
    return a_prev.sqrt() * pred_x0 + (1. - a_prev - sigma ** 2).sqrt() * e, pred_x0


class PLMSSampler(object):
    def __init__(self, model, schedule="linear", **kwargs):
        super().__init__()
        self.model = model
        self.ddpm_num_timesteps = model.num_timesteps
        self.schedule = schedule
        # capture one multistep iteration (set time, model, fused update, tick) as a hipGraph and replay it; False: all eager
        self.use_graph = True
        self.batch_cfg = True               # both guidance passes as one batch of 2B
        self.hoist_hint_encode = True       # VAE-encode a condition image once per sample() call (ControlLDM.hint_cache)

    def register_buffer(self, name, attr):
        if isinstance(attr, torch.Tensor) and attr.device != self.model.device:
            attr = attr.to(self.model.device)
        setattr(self, name, attr)

    def make_schedule(self, ddim_num_steps, ddim_discretize="uniform", ddim_eta=0., verbose=True):
        if ddim_eta != 0:
            raise ValueError('ddim_eta must be 0 for PLMS')
        self.ddim_timesteps = make_ddim_timesteps(ddim_discr_method=ddim_discretize, num_ddim_timesteps=ddim_num_steps,
                                                  num_ddpm_timesteps=self.ddpm_num_timesteps, verbose=verbose)
        alphas_cumprod = self.model.alphas_cumprod
        assert alphas_cumprod.shape[0] == self.ddpm_num_timesteps, "alphas have to be defined for each timestep"
        to_torch = lambda x: x.clone().detach().to(torch.float32).to(self.model.device)
        self.register_buffer("betas", to_torch(self.model.betas))
        self.register_buffer("alphas_cumprod", to_torch(alphas_cumprod))
        self.register_buffer("alphas_cumprod_prev", to_torch(self.model.alphas_cumprod_prev))
        ac = alphas_cumprod.cpu()
        self.register_buffer("sqrt_alphas_cumprod", to_torch(np.sqrt(ac)))
        self.register_buffer("sqrt_one_minus_alphas_cumprod", to_torch(np.sqrt(1. - ac)))
        ddim_sigmas, ddim_alphas, ddim_alphas_prev = make_ddim_sampling_parameters(
            alphacums=ac, ddim_timesteps=self.ddim_timesteps, eta=ddim_eta, verbose=verbose)
        self.register_buffer("ddim_sigmas", ddim_sigmas)
        self.register_buffer("ddim_alphas", ddim_alphas)
        self.register_buffer("ddim_alphas_prev", ddim_alphas_prev)
        self.register_buffer("ddim_sqrt_one_minus_alphas", np.sqrt(1. - ddim_alphas))
        # DDIMSampler's device table: rows = ddim index, cols = {a_t, a_prev, sigma_t, sqrt(1-a_t)}; each entry is the fp32
        # value torch.full(..., table[index]) produces in the reference (plms.py:207-210)
        cols = [torch.as_tensor(np.asarray(v, dtype=np.float64) if not torch.is_tensor(v) else v.double().cpu().numpy())
                for v in (ddim_alphas, ddim_alphas_prev, ddim_sigmas, np.sqrt(1. - ddim_alphas))]
        self.coef_table = torch.stack([c.to(torch.float32) for c in cols], dim=1).contiguous().to(self.model.device)

    @torch.no_grad()
    def sample(self, S, batch_size, shape, conditioning=None, callback=None, normals_sequence=None, img_callback=None,
               quantize_x0=False, eta=0., mask=None, x0=None, temperature=1., noise_dropout=0., score_corrector=None,
               corrector_kwargs=None, verbose=True, x_T=None, log_every_t=100, unconditional_guidance_scale=1.,
               unconditional_conditioning=None, dynamic_threshold=None, **kwargs):
        self.make_schedule(ddim_num_steps=S, ddim_eta=eta, verbose=verbose)
        C, H, W = shape
        size = (batch_size, C, H, W)
        if verbose:
            print(f"Data shape for PLMS sampling is {size}")
        with hint_scope(self.model, self.hoist_hint_encode):
            return self.plms_sampling(conditioning, size, callback=callback, img_callback=img_callback,
                                      quantize_denoised=quantize_x0, mask=mask, x0=x0, ddim_use_original_steps=False,
                                      noise_dropout=noise_dropout, temperature=temperature,
                                      score_corrector=score_corrector, corrector_kwargs=corrector_kwargs, x_T=x_T,
                                      log_every_t=log_every_t, unconditional_guidance_scale=unconditional_guidance_scale,
                                      unconditional_conditioning=unconditional_conditioning,
                                      dynamic_threshold=dynamic_threshold)

    def _refuse(self, use_original_steps, quantize_denoised, score_corrector, dynamic_threshold):
        if use_original_steps or quantize_denoised or score_corrector is not None or dynamic_threshold is not None:
            raise NotImplementedError("option not used by the CtrLoRA sampling scripts")
        if getattr(self.model, "parameterization", "eps") != "eps":
            raise NotImplementedError("v-parameterisation is not used by the CtrLoRA configs")

    @torch.no_grad()
    def plms_sampling(self, cond, shape, x_T=None, ddim_use_original_steps=False, callback=None, timesteps=None,
                      quantize_denoised=False, mask=None, x0=None, img_callback=None, log_every_t=100, temperature=1.,
                      noise_dropout=0., score_corrector=None, corrector_kwargs=None, unconditional_guidance_scale=1.,
                      unconditional_conditioning=None, dynamic_threshold=None):
        self._refuse(ddim_use_original_steps, quantize_denoised, score_corrector, dynamic_threshold)
        device = self.model.betas.device
        img = torch.randn(shape, device=device) if x_T is None else x_T.to(device).float()
        if timesteps is None:
            timesteps = self.ddim_timesteps
        else:
            subset_end = int(min(timesteps / self.ddim_timesteps.shape[0], 1) * self.ddim_timesteps.shape[0]) - 1
            timesteps = self.ddim_timesteps[:subset_end]
        S = int(timesteps.shape[0])
        intermediates = {"x_inter": [img], "pred_x0": [img]}
        scale = float(unconditional_guidance_scale)
        uncond = None if scale == 1. else unconditional_conditioning       # None: no guidance, one pass
        both = batch_conds(cond, uncond, UNCOND_FIRST, cat_tensors=True) if self.batch_cfg else None
        if mask is not None:
            assert x0 is not None

        def after_step(i, x, pred_x0, copy):
            if callback:
                callback(i)
            if img_callback:
                img_callback(pred_x0, i)
            index = S - i - 1
            if index % log_every_t == 0 or index == S - 1:
                intermediates["x_inter"].append(x.clone() if copy else x)
                intermediates["pred_x0"].append(pred_x0.clone() if copy else pred_x0)

        run = (cond, uncond, both, scale, timesteps, after_step)
        if not img.is_cuda:
            x = self._loop_torch(img, mask, x0, *run)
        elif self.use_graph and S >= 4 and mask is None and engine_of(self.model) is not None:
            x = self._loop_graphed(img, *run)
        else:
            x = self._loop_eager(img, mask, x0, *run)
        return x, intermediates

    def _times(self, timesteps, i, b, device):
        """(t, t_next) of iteration i as (b,) long tensors: flip(timesteps)[i] and flip(timesteps)[min(i + 1, S - 1)]."""
        S = timesteps.shape[0]
        full = lambda k: torch.full((b,), int(timesteps[S - 1 - k]), device=device, dtype=torch.long)
        return full(i), full(min(i + 1, S - 1))

    # ------------------------------------------------------------------ tensors outside the engine
    def _loop_torch(self, img, mask, x0, cond, uncond, both, scale, timesteps, after_step):
        x, S, old_eps = img.float(), timesteps.shape[0], []
        for i in range(S):
            ts, ts_next = self._times(timesteps, i, x.shape[0], x.device)
            if mask is not None:
                x = self.model.q_sample(x0, ts) * mask + (1. - mask) * x
            x, pred_x0, e = self._p_sample_torch(x, cond, uncond, both, scale, ts, ts_next, S - 1 - i, old_eps)
            old_eps = (old_eps + [e])[-3:]
            after_step(i, x, pred_x0, False)
        return x

    def _p_sample_torch(self, x, cond, uncond, both, scale, ts, ts_next, index, old_eps):
        row = self.coef_table[index].to(x.device)

        def eps(x_, t_):
            e_c, e_u = guided_eps(self.model, x_, t_, cond, uncond, both, UNCOND_FIRST)
            return e_c.float() if e_u is None else e_u.float() + scale * (e_c.float() - e_u.float())

        e = eps(x, ts)
        if len(old_eps) == 0:
            e_prime = (e + eps(_update(x, e, row)[0], ts_next)) / 2
        else:
            e_prime = _combine(e, old_eps)
        x_prev, pred_x0 = _update(x, e_prime, row)
        return x_prev, pred_x0, e

    # ------------------------------------------------------------------ GPU
    def _state(self, img, S):
        x = img.float().contiguous().clone()
        hist = torch.empty((4, x.numel()), dtype=torch.float32, device=x.device)
        return x, torch.empty_like(x), hist, self.coef_table[:S].contiguous().to(x.device)

    def _eps(self, x, ts, cond, uncond, both):
        e_c, e_u = guided_eps(self.model, x, ts, cond, uncond, both, UNCOND_FIRST)
        return e_c.float().contiguous(), None if e_u is None else e_u.float().contiguous()

    def _start(self, x, pred_x0, hist, coef, ts, ts_next, cond, uncond, both, scale):
        """Iteration 0, in place on x: the predictor from e(x, t_0), a second evaluation at (predictor, t_1), the update."""
        from ctrlora_amd import hip
        e_c, e_u = self._eps(x, ts, cond, uncond, both)
        x_pred = hip.plms_step(x, e_c, e_u, coef, 0, hip.PLMS_START, scale, hist, torch.empty_like(x))
        e_c, e_u = self._eps(x_pred, ts_next, cond, uncond, both)
        hip.plms_step(x, e_c, e_u, coef, 0, hip.PLMS_FINISH, scale, hist, x, pred_x0)

    def _loop_eager(self, img, mask, x0, cond, uncond, both, scale, timesteps, after_step):
        """Every iteration from Python: S + 1 model calls."""
        from ctrlora_amd import hip
        S = int(timesteps.shape[0])
        x, pred_x0, hist, coef = self._state(img, S)
        with context_kv(engine_of(self.model)):
            for i in range(S):
                ts, ts_next = self._times(timesteps, i, x.shape[0], x.device)
                if mask is not None:
                    x = (self.model.q_sample(x0, ts) * mask + (1. - mask) * x).float().contiguous()
                if i == 0:
                    self._start(x, pred_x0, hist, coef, ts, ts_next, cond, uncond, both, scale)
                else:
                    e_c, e_u = self._eps(x, ts, cond, uncond, both)
                    hip.plms_step(x, e_c, e_u, coef, i, hip.PLMS_MULTISTEP, scale, hist, x, pred_x0)
                after_step(i, x, pred_x0, True)
        return x

    def _loop_graphed(self, img, cond, uncond, both, scale, timesteps, after_step):
        """Iteration 0 by hand (its two evaluations fill the context K/V cache), then the loop state on the device, as
        DDIMSampler._sampling_graphed: a cursor i counts iterations, cl_ddim_set_t derives ts = ddim_timesteps[S-1-i],
        cl_plms_step_dev the table row, the ring slots and the order.  guided_loop.run_steps runs iteration 1 eagerly, captures
        iteration 2 and replays that capture for the rest."""
        from ctrlora_amd import hip
        S, b = int(timesteps.shape[0]), img.shape[0]
        x, pred_x0, hist, coef = self._state(img, S)
        ts = torch.zeros(b, dtype=torch.long, device=x.device)
        cursor = torch.zeros(1, dtype=torch.int32, device=x.device)
        table = torch.as_tensor(np.ascontiguousarray(timesteps).astype(np.int64)).to(x.device)

        def body():
            hip.ddim_set_t(table, cursor, S, ts)
            e_c, e_u = self._eps(x, ts, cond, uncond, both)
            hip.plms_step_dev(x, e_c, e_u, coef, cursor, S, scale, hist, x, pred_x0)
            hip.tick(cursor)

        with context_kv(engine_of(self.model)):
            self._start(x, pred_x0, hist, coef, *self._times(timesteps, 0, b, x.device), cond, uncond, both, scale)
            hip.tick(cursor)
            after_step(0, x, pred_x0, True)
            run_steps(body, S - 1, lambda j: after_step(j + 1, x, pred_x0, True))   # has waited for the last replay
            return x.clone()

    @torch.no_grad()
    def p_sample_plms(self, x, c, t, index, repeat_noise=False, use_original_steps=False, quantize_denoised=False,
                      temperature=1., noise_dropout=0., score_corrector=None, corrector_kwargs=None,
                      unconditional_guidance_scale=1., unconditional_conditioning=None, old_eps=None, t_next=None,
                      dynamic_threshold=None):
        """One iteration on table row `index`; the order follows len(old_eps) (0: the two-evaluation start, which needs
        t_next).  Returns (x_prev, pred_x0, e_t)."""
        self._refuse(use_original_steps, quantize_denoised, score_corrector, dynamic_threshold)
        scale = float(unconditional_guidance_scale)
        uncond = None if scale == 1. else unconditional_conditioning
        both = batch_conds(c, uncond, UNCOND_FIRST, cat_tensors=True) if self.batch_cfg else None
        old_eps = list(old_eps or [])[-3:]
        if not x.is_cuda:
            return self._p_sample_torch(x.float(), c, uncond, both, scale, t, t_next, index, old_eps)
        from ctrlora_amd import hip
        x = x.float().contiguous()
        k = len(old_eps)
        # iteration k of a (k + 1)-row table reads row 0: the row this call names, with the order its history gives
        coef = self.coef_table[index:index + 1].to(x.device).repeat(k + 1, 1).contiguous()
        hist = torch.empty((4, x.numel()), dtype=torch.float32, device=x.device)
        for j in range(1, k + 1):
            hist[k - j].copy_(old_eps[-j].reshape(-1))
        x_prev, pred_x0 = torch.empty_like(x), torch.empty_like(x)
        if k == 0:
            x_prev.copy_(x)
            self._start(x_prev, pred_x0, hist, coef, t, t_next, c, uncond, both, scale)
        else:
            e_c, e_u = self._eps(x, t, c, uncond, both)
            hip.plms_step(x, e_c, e_u, coef, k, hip.PLMS_MULTISTEP, scale, hist, x_prev, pred_x0)
        return x_prev, pred_x0, hist[k].view_as(x).clone()
