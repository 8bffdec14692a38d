"""Golden vectors for ControlNetFinetune's `norm_trainable` / `zero_trainable` switches, from the UNMODIFIED reference
(run in the build container only; see make_golden.py for how the reference is imported).

    python tests/golden/make_golden_flags.py      # writes tests/golden/flags_tiny.pt

For each of (norm_trainable, zero_trainable) = (False, True), (True, False), (False, False) at the `tiny` configuration the
real ControlFinetuneLDM is built with those constructor kwargs, loaded with the key-addressed weights (oracle/arch.py:
draw_param -- the zero convs are NON-zero, as after Base-ControlNet pre-training, otherwise the ControlNet contributes
nothing and every gradient below is trivially zero), and run through configure_optimizers() -> p_losses -> backward -> one
AdamW step.  Recorded per combination:

  trainable_names   the optimizer's parameters, in the reference's order
  eps, loss         apply_model / p_losses on the seeded inputs
  grad_digest       digest() of every selected gradient
  grad_vals         N_SAMPLED evenly spaced entries of every selected gradient (index rule: sample_idx below) + l2 + sum
  adamw_digest      digest() of every ~24th selected parameter after the step
  frozen_digest     digest() of a fixed sample of NON-selected ControlNet tensors after the step, next to the digest of
                    their initial value (the generator asserts they are equal: untouched, weight decay included)
"""
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.dont_write_bytecode = True

import make_golden as mg  # noqa: E402
from make_golden import build_ldm, digest, install_stubs, use_reference_packages  # noqa: E402

COMBOS = ((False, True), (True, False), (False, False))
N_SAMPLED = 128
B, H, SEED, LR = 2, 16, 23, 1e-4


def combo_key(norm_trainable: bool, zero_trainable: bool) -> str:
    return f"norm{int(norm_trainable)}_zero{int(zero_trainable)}"


def sample_idx(numel: int, n: int = N_SAMPLED) -> torch.Tensor:
    return torch.linspace(0, numel - 1, min(n, numel)).long()


def gen_flags_golden(cfg, norm_trainable, zero_trainable):
    from oracle import arch
    base_kwargs = mg.ref_kwargs

    def kwargs_with_flags(c, control):
        kw = base_kwargs(c, control)
        if control:
            kw.update(norm_trainable=norm_trainable, zero_trainable=zero_trainable)
        return kw

    mg.ref_kwargs = kwargs_with_flags
    try:
        torch.manual_seed(0)
        model = build_ldm(cfg)
    finally:
        mg.ref_kwargs = base_kwargs
    cm = model.control_model
    assert (cm.norm_trainable, cm.zero_trainable) == (norm_trainable, zero_trainable)
    init = arch.make_state(arch.controlnet_shapes(cfg), SEED)
    cm.load_state_dict(init, strict=True)
    model.model.diffusion_model.load_state_dict(arch.make_state(arch.unet_shapes(cfg), SEED), strict=True)
    model.train()
    model.learning_rate = LR
    inp = mg.inputs_for(cfg, B, H, SEED)
    cond = dict(c_crossattn=[inp["ctx"]], c_concat=[inp["hint_z"]])
    os.makedirs("./tmp", exist_ok=True)
    opt = model.configure_optimizers()
    loss, _ = model.p_losses(inp["z"], cond, inp["t"], noise=inp["noise"])
    with torch.no_grad():
        eps = model.apply_model(model.q_sample(inp["z"], inp["t"], inp["noise"]), inp["t"], cond)
    loss.backward()
    params = dict(cm.named_parameters())
    by_id = {id(p): n for n, p in params.items()}
    tr = [by_id[id(p)] for p in opt.param_groups[0]["params"]]
    with open("./tmp/finetune_trainable_params.txt") as f:
        assert f.read().split() == tr
    out = dict(trainable_names=tr, eps=eps.clone(), loss=float(loss), grad_digest={}, grad_vals={})
    for n in tr:
        g = params[n].grad
        assert g is not None and float(g.norm()) > 0.0, f"{n}: zero gradient -- the fixture would test nothing"
        f = g.detach().float().flatten()
        out["grad_digest"][n] = digest(g)
        out["grad_vals"][n] = dict(vals=f[sample_idx(f.numel())].clone(), l2=float(f.double().norm()),
                                   sum=float(f.double().sum()))
    opt.step()
    out["adamw_digest"] = {n: digest(params[n]) for n in tr[:: max(1, len(tr) // 24)]}
    sel = set(tr)
    excluded = [n for n in params if n not in sel and ("norm" in n or "zero_convs" in n or "middle_block_out" in n)]
    others = [n for n in params if n not in sel and n not in set(excluded)]
    pick = excluded[:: max(1, len(excluded) // 16)] + others[:: max(1, len(others) // 8)]
    out["frozen_digest"] = {}
    for n in pick:
        assert torch.equal(params[n].detach(), init[n]), f"{n} moved although it is not in the optimizer"
        out["frozen_digest"][n] = dict(after=digest(params[n]), initial=digest(init[n]))
    print(f"[golden] flags {combo_key(norm_trainable, zero_trainable)}: loss={out['loss']:.6f} trainables={len(tr)} "
          f"frozen sample={len(pick)}")
    return out


if __name__ == "__main__":
    assert os.path.isdir(mg.REF), "run in the build container (needs the reference checkout)"
    install_stubs()
    os.chdir("/tmp")
    use_reference_packages()
    from oracle import arch
    cfg = arch.TINY
    out = dict(meta=dict(name="tiny", B=B, H=H, seed=SEED, lr=LR, n_sampled=N_SAMPLED, cfg=cfg.__dict__), combos={})
    for nt, zt in COMBOS:
        out["combos"][combo_key(nt, zt)] = gen_flags_golden(cfg, nt, zt)
    path = f"{HERE}/flags_tiny.pt"
    torch.save(out, path)
    print(f"[golden] flags_tiny.pt written: {os.path.getsize(path) / 1e6:.2f} MB")
