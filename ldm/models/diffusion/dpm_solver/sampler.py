"""DPM-Solver++ sampler (API of the reference's ldm/models/diffusion/dpm_solver/sampler.py: DPMSolverSampler.sample; the
solver it configures there is dpm_solver.py's DPM_Solver with predict_x0=True, method="multistep", order=2,
skip_type="time_uniform", lower_order_final=True -- Lu et al., "DPM-Solver++", arXiv:2211.01095).

What changes underneath, not in the results:
  * the multistep update is a linear recurrence over the last (up to) three x0 predictions m_k:
        x_{i+1} = cx_i x_i + c0_i m_i + c1_i m_{i-1} + c2_i m_{i-2},       m_i = (x_i - sigma_i eps_i) / alpha_i.
    Its coefficients depend on the time grid only, so they are computed ONCE on the host (fp64, stored fp32) into a
    [S][8] table {alpha_i, sigma_i, cx_i, c0_i, c1_i, c2_i, t_in_i, 0}; guidance + x0 prediction + history write + update
    are one fused HIP kernel per step (cl_dpmpp_step) where the reference issues about a dozen elementwise launches;
  * the model is evaluated at NON-INTEGER times t_in = (t - 1/N) * 1000 (999, 949.05, 899.1, ... for 20 steps); the engine
    embeds them in floating point (cl_timestep_embedding_f);
  * classifier-free guidance is one batch of 2B ordered [unconditional; conditional] as the reference batches it, for
    tensors AND for same-structure dict conditionings (the reference's torch.cat would raise on ControlLDM's dicts);
  * with an engine model the step index, the model time and the history slot live on the device, and one step
    (cl_dpm_set_t, apply_model, cl_dpmpp_step_dev, cl_tick) is captured as a hipGraph and replayed.
Tensors outside the engine (CPU) take the same table through a plain-torch update.
"""
import numpy as np
import torch

from ldm.models.diffusion.guided_loop import UNCOND_FIRST, batch_conds, context_kv, engine_of, guided_eps, hint_scope, run_steps


def dpmpp_table(alphas_cumprod, S, order=2, skip_type="time_uniform"):
    """The time grid and the coefficient table of the multistep solver, fp64 on the host.

    log_alpha(t) is the piecewise-linear interpolation of 0.5 log(alphas_cumprod) over t_k = k / N, k = 1..N
    (NoiseScheduleVP('discrete')); alpha = exp(log_alpha), sigma = sqrt(1 - alpha^2), lambda = log_alpha - log(sigma).
    Step i -> i + 1 with h = lambda_{i+1} - lambda_i, phi = expm1(-h), a = alpha_{i+1}, and r0 = (lambda_i - lambda_{i-1}) / h,
    r1 = (lambda_{i-1} - lambda_{i-2}) / h:
        order 1:  x' = cx x - a phi m_i
        order 2:  x' = cx x - a phi m_i - 0.5 a phi D1_0,                     D1_0 = (m_i - m_{i-1}) / r0
        order 3:  x' = cx x - a phi m_i + a (phi / h + 1) D1 - a ((phi + h) / h^2 - 0.5) D2,
                  D1_1 = (m_{i-1} - m_{i-2}) / r1,  D1 = D1_0 + r0 / (r0 + r1) (D1_0 - D1_1),  D2 = (D1_0 - D1_1) / (r0 + r1)
    expanded into the coefficients of m_i, m_{i-1}, m_{i-2}.  The order of step i is min(order, i + 1) (start-up) and, for
    S < 15, also min(., S - i) (lower_order_final).  Returns (times fp64 [S + 1], table fp64 [S][8], orders)."""
    if order not in (1, 2, 3):
        raise ValueError(f"Solver order must be 1 or 2 or 3, got {order}")
    if skip_type == "logSNR":
        raise NotImplementedError("skip_type='logSNR' is not implemented (time_uniform / time_quadratic are)")
    if skip_type not in ("time_uniform", "time_quadratic"):
        raise ValueError(f"Unsupported skip_type {skip_type}, need to be 'time_uniform' or 'time_quadratic'")
    S = int(S)
    if S < order:
        raise ValueError(f"the multistep solver of order {order} needs at least {order} steps, got {S}")
    ac = np.asarray(alphas_cumprod.detach().cpu().double().numpy() if torch.is_tensor(alphas_cumprod) else alphas_cumprod,
                    dtype=np.float64)
    N = ac.shape[0]
    t_k = np.arange(1, N + 1, dtype=np.float64) / N
    if skip_type == "time_uniform":
        t = np.linspace(1.0, 1.0 / N, S + 1)
    else:
        t = np.linspace(1.0, (1.0 / N) ** 0.5, S + 1) ** 2
    log_alpha = np.interp(t, t_k, 0.5 * np.log(ac))
    alpha = np.exp(log_alpha)
    sigma = np.sqrt(1.0 - np.exp(2.0 * log_alpha))
    lam = log_alpha - np.log(sigma)
    table = np.zeros((S, 8), dtype=np.float64)
    orders = []
    for i in range(S):
        p = min(order, i + 1)
        if S < 15:
            p = min(p, S - i)
        orders.append(p)
        h = lam[i + 1] - lam[i]
        phi = np.expm1(-h)
        a = alpha[i + 1]
        c0, c1, c2 = -a * phi, 0.0, 0.0
        if p == 2:
            r0 = (lam[i] - lam[i - 1]) / h
            c0, c1 = -a * phi * (1.0 + 0.5 / r0), a * phi * 0.5 / r0
        elif p == 3:
            r0, r1 = (lam[i] - lam[i - 1]) / h, (lam[i - 1] - lam[i - 2]) / h
            A, Bc = a * (phi / h + 1.0), a * ((phi + h) / h ** 2 - 0.5)
            q, s = r0 / (r0 + r1), 1.0 / (r0 + r1)
            u0, u1 = A * (1.0 + q) - Bc * s, -A * q + Bc * s          # weights of D1_0 and D1_1
            c0, c1, c2 = -a * phi + u0 / r0, -u0 / r0 + u1 / r1, -u1 / r1
        table[i] = (alpha[i], sigma[i], sigma[i + 1] / sigma[i], c0, c1, c2, (t[i] - 1.0 / N) * 1000.0, 0.0)
    return t, table, orders


class DPMSolverSampler(object):
    def __init__(self, model, **kwargs):
        super().__init__()
        self.model = model
        to_torch = lambda x: x.clone().detach().to(torch.float32).to(model.device)
        self.register_buffer("alphas_cumprod", to_torch(model.alphas_cumprod))
        self.order = 2                      # 1 / 2 / 3
        self.skip_type = "time_uniform"     # or "time_quadratic"
        # capture one step (set time, model, fused update, tick) as a hipGraph and replay it; False: every step eager
        self.use_graph = True
        self.batch_cfg = True               # both guidance passes as one batch of 2B
        self.hoist_hint_encode = True       # VAE-encode a condition image once per sample() call (ControlLDM.hint_cache)

    def register_buffer(self, name, attr):
        if isinstance(attr, torch.Tensor) and attr.device != self.model.device:
            attr = attr.to(self.model.device)
        setattr(self, name, attr)

    def make_schedule(self, S):
        self.timesteps, table, self.step_orders = dpmpp_table(self.alphas_cumprod, S, self.order, self.skip_type)
        self.coef_table = torch.as_tensor(table).to(torch.float32).contiguous()      # host copy, fp32

    @torch.no_grad()
    def sample(self, S, batch_size, shape, conditioning=None, callback=None, normals_sequence=None, img_callback=None,
               quantize_x0=False, eta=0., mask=None, x0=None, temperature=1., noise_dropout=0., score_corrector=None,
               corrector_kwargs=None, verbose=True, x_T=None, log_every_t=100, unconditional_guidance_scale=1.,
               unconditional_conditioning=None, **kwargs):
        """Returns (x, None).  As in the reference, only S, batch_size, shape, conditioning, x_T and the two guidance
        arguments act; everything else is accepted and ignored (verbose only silences the banner)."""
        if getattr(self.model, "parameterization", "eps") != "eps":
            raise NotImplementedError("v-parameterisation is not used by the CtrLoRA configs")
        self.make_schedule(S)
        C, H, W = shape
        size = (batch_size, C, H, W)
        if verbose:
            print(f"Data shape for DPM-Solver sampling is {size}, sampling steps {S}")
        device = self.model.betas.device
        img = torch.randn(size, device=device) if x_T is None else x_T.to(device)
        cond, scale = conditioning, float(unconditional_guidance_scale)
        uncond = None if scale == 1. else unconditional_conditioning       # None: no guidance, one pass
        both = batch_conds(cond, uncond, UNCOND_FIRST, cat_tensors=True) if self.batch_cfg else None
        with hint_scope(self.model, self.hoist_hint_encode):
            if not img.is_cuda:
                x = self._loop_torch(img, cond, uncond, both, scale)
            elif self.use_graph and int(S) >= 4 and engine_of(self.model) is not None:
                x = self._loop_graphed(img, cond, uncond, both, scale)
            else:
                x = self._loop_eager(img, cond, uncond, both, scale)
        return x, None

    # ------------------------------------------------------------------ tensors outside the engine
    def _loop_torch(self, img, cond, uncond, both, scale):
        x = img.float()
        S, tab = self.coef_table.shape[0], self.coef_table
        nb = x.shape[0] * (2 if both is not None else 1)
        hist = [None, None, None]
        for i in range(S):
            alpha, sigma, cx, c0, c1, c2, t_in = (tab[i, k] for k in range(7))
            ts = torch.full((nb,), float(t_in), dtype=torch.float32, device=x.device)
            e_c, e_u = guided_eps(self.model, x, ts, cond, uncond, both, UNCOND_FIRST)
            e = e_c.float() if e_u is None else e_u.float() + scale * (e_c.float() - e_u.float())
            m = (x - sigma * e) / alpha
            hist[i % 3] = m
            x = cx * x + c0 * m
            if float(c1) != 0.0:
                x = x + c1 * hist[(i + 2) % 3]
            if float(c2) != 0.0:
                x = x + c2 * hist[(i + 1) % 3]
        return x

    # ------------------------------------------------------------------ GPU, every step eager
    def _state(self, img, both):
        x = img.float().contiguous().clone()
        nb = x.shape[0] * (2 if both is not None else 1)
        hist = torch.empty((3, x.numel()), dtype=torch.float32, device=x.device)
        return x, torch.empty_like(x), hist, nb, self.coef_table.to(x.device)

    def _loop_eager(self, img, cond, uncond, both, scale):
        from ctrlora_amd import hip
        x, pred_x0, hist, nb, coef = self._state(img, both)
        with context_kv(engine_of(self.model)):
            for i in range(coef.shape[0]):
                ts = torch.full((nb,), float(self.coef_table[i, 6]), dtype=torch.float32, device=x.device)
                e_c, e_u = guided_eps(self.model, x, ts, cond, uncond, both, UNCOND_FIRST)
                hip.dpmpp_step(x, e_c.float().contiguous(), None if e_u is None else e_u.float().contiguous(), coef, i, scale,
                               hist, x, pred_x0)
        return x

    # ------------------------------------------------------------------ GPU, one captured step replayed
    def _loop_graphed(self, img, cond, uncond, both, scale):
        """Loop state on the device, as DDIMSampler._sampling_graphed: a cursor i counts iterations, cl_dpm_set_t writes the
        model time of row i, cl_dpmpp_step_dev reads row i and the history slots i % 3, (i + 2) % 3, (i + 1) % 3.  One step is
        then a fixed kernel sequence: guided_loop.run_steps captures it once and replays it."""
        from ctrlora_amd import hip
        x, pred_x0, hist, nb, coef = self._state(img, both)
        S = coef.shape[0]
        ts = torch.zeros(nb, dtype=torch.float32, device=x.device)
        cursor = torch.zeros(1, dtype=torch.int32, device=x.device)

        def body():
            hip.dpm_set_t(coef, cursor, S, ts)
            e_c, e_u = guided_eps(self.model, x, ts, cond, uncond, both, UNCOND_FIRST)
            hip.dpmpp_step_dev(x, e_c.float().contiguous(), None if e_u is None else e_u.float().contiguous(), coef, cursor, S,
                               scale, hist, x, pred_x0)
            hip.tick(cursor)

        with context_kv(engine_of(self.model)):
            run_steps(body, S)      # keeps no graph: it has waited for the last replay when it returns
            return x.clone()
