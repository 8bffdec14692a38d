"""Golden vectors for the EMA of trained weights, from the UNMODIFIED reference's ldm/modules/ema.py:LitEma.

    python tests/golden/make_golden_ema.py /path/to/reference          # writes tests/golden/ema.pt (a few KB)

A toy module -- parameters of shapes (5,), (3, 4), (2, 2, 3, 3) and one requires_grad=False parameter LitEma must ignore --
is shadowed by LitEma and updated 12 times in each of three runs; between updates a seeded random walk moves every trainable
parameter.  Stored per run: the parameters at every update, every shadow after every update, num_updates after every update.

    defaults   decay 0.9999, warm-up on: d = (1 + u) / (10 + u) throughout
    no_warmup  use_num_upates=False, decay 0.9: d = decay, num_updates stays -1
    crossing   decay 0.9999, num_updates preset to 89 985: (1 + u) / (10 + u) reaches the 0.9999 cap at u = 89 990, inside the run

Values are normal-range randn draws: nothing rests on denormal handling.
"""
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True

UPDATES = 12
RUNS = dict(defaults=dict(decay=0.9999, use_num_updates=True, preset=None, seed=101),
            no_warmup=dict(decay=0.9, use_num_updates=False, preset=None, seed=102),
            crossing=dict(decay=0.9999, use_num_updates=True, preset=89985, seed=103))


class Toy(torch.nn.Module):
    def __init__(self, seed):
        super().__init__()
        g = torch.Generator().manual_seed(seed)
        mk = lambda *s: torch.nn.Parameter(torch.randn(*s, generator=g))
        self.bias = mk(5)
        self.proj = torch.nn.Linear(4, 3, bias=False)
        self.proj.weight = mk(3, 4)
        self.conv = torch.nn.Conv2d(2, 2, 3, bias=False)
        self.conv.weight = mk(2, 2, 3, 3)
        self.frozen = torch.nn.Parameter(torch.randn(4, generator=g), requires_grad=False)


def walk(toy, gen):
    """The move between two updates: every parameter (the frozen one too) takes a seeded step of about a tenth of its size."""
    with torch.no_grad():
        for p in toy.parameters():
            p.add_(0.1 * torch.randn(p.shape, generator=gen))


def main():
    ref = sys.argv[1]
    sys.path.insert(0, ref)
    from ldm.modules.ema import LitEma
    out = {}
    for name, cfg in RUNS.items():
        toy = Toy(cfg["seed"])
        ema = LitEma(toy, decay=cfg["decay"], use_num_upates=cfg["use_num_updates"])
        if cfg["preset"] is not None:
            ema.num_updates.fill_(cfg["preset"])
        gen = torch.Generator().manual_seed(cfg["seed"] + 1000)
        rec = dict(cfg=dict(cfg), names=dict(ema.m_name2s_name), init={n: p.detach().clone() for n, p in toy.named_parameters()},
                   params=[], shadows=[], num_updates=[])
        for _ in range(UPDATES):
            walk(toy, gen)
            ema(toy)
            rec["params"].append({n: p.detach().clone() for n, p in toy.named_parameters()})
            rec["shadows"].append({k: b.detach().clone() for k, b in ema.named_buffers() if k not in ("decay", "num_updates")})
            rec["num_updates"].append(int(ema.num_updates))
        assert "frozen" not in rec["names"]
        out[name] = rec
    crossing = out["crossing"]["num_updates"]
    assert crossing[0] == 89986 and crossing[-1] == 89997 and 89990 in crossing
    path = os.path.join(HERE, "ema.pt")
    torch.save(out, path)
    print(f"wrote {path} ({os.path.getsize(path)} bytes)")


if __name__ == "__main__":
    main()
