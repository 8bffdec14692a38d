"""`Trainer.fit` with Min-SNR weights and the Huber loss on an MI355X: the replayed step is the eager loop's step.

Model, batches and seeds are those of tests/test_gpu_trainer_graph.py (tiny fine-tune model, B = 2, latent 16 x 16, lr 1e-3,
log_every_n_steps = 1), with min_snr_gamma = 5 and loss_type "huber".  Five optimizer steps, once through the eager loop (autograd:
PLossFn) and once with graph_step=True (engine_train_step, captured): the same seed gives the same logged losses and the same
final control_model parameters, bit for bit, and graph_replays > 0.  In fp32 the weight gradients run in their opt-in fixed-order
form (hip.WGRAD_F32_DETERMINISTIC, as in tests/test_gpu_latent_cache.py).  With accumulate_grad_batches = 2 the eager leg multiplies
d loss / d eps by 1 / 2 after the kernel and the replayed leg inside it: a power of two, the same bits.

Bits can be compared only where the engine itself repeats them.  Measured on one MI355X with this file's _fit, the loss feature OFF
(plain l2, the parent's launches), two eager fits from one seed: at accumulate_grad_batches = 1 bit-equal in fp32 and bf16 (losses
and all 488 control_model tensors, five steps); at 2 NOT -- after ONE optimizer step in fp32 five tensors differ, all of them the
GroupNorm biases of transformer blocks (input_blocks.{2,4,7,8}.1.norm.bias, middle_block.1.norm.bias, by 1e-10 .. 2e-9: their
gradient is added onto the first micro-batch's with atomicAdd, one per sample's workgroup, in arrival order: csrc/norm.hip), after five steps 246 of 488 (rel-L2
4e-7, losses in their last bit) and in bf16 1 .. 2 of 488 (rel-L2 3e-9 .. 1e-8).  Graph against eager shows the same figures with
the feature off and on.  So at accumulate_grad_batches = 2 the bit comparison runs on the model with `norm_trainable: False`
(the supported frozen-norm fine-tune of tests/test_gpu_flags.py: no norm gradient is formed), and the default model is held to
the same-trajectory gate of tests/test_gpu_trainer_graph.py (losses 1e-4 relative, parameters rel-L2 1e-4) there.

Last, set_loss_weights between two replays: the next step's loss follows the new table, with no new capture."""
import pytest
import torch

pytestmark = pytest.mark.gpu

B, H, CTX_DIM, SEED, STEPS = 2, 16, 96, 7, 5


@pytest.fixture(autouse=True)
def _setup(tmp_path, monkeypatch):
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from ctrlora_amd import hip
    hip.lib()
    monkeypatch.setattr(hip, "WGRAD_F32_DETERMINISTIC", True)
    monkeypatch.chdir(tmp_path)          # configure_optimizers writes ./tmp/finetune_trainable_params.txt, the trainer ./run


def _batches(n, seed=5):
    g = torch.Generator().manual_seed(seed)
    mk = lambda *s: torch.randn(*s, generator=g).cuda()
    return [dict(z=mk(B, 4, H, H), ctx=mk(B, 77, CTX_DIM), hint_z=mk(B, 4, H, H) * 0.9) for _ in range(n)]


def _model(norm_trainable=True, **params):
    import bench

    def mutate(p):
        p.update(params)
        p["control_stage_config"]["params"].update(norm_trainable=norm_trainable)
    m = bench.build_model("ctrlora_finetune_sd15_rank128.yaml", 0, tiny=True, mutate=mutate)
    m.learning_rate = 1e-3
    m.get_input = lambda batch, k, *a, **kw: (batch["z"], {"c_crossattn": [batch["ctx"]], "c_concat": [batch["hint_z"]]})
    return m


def _fit(graph_step, acc=1, precision=32, callbacks=(), **params):
    from ctrlora_amd.trainer import Trainer
    m = _model(**params)
    tr = Trainer(max_steps=STEPS, accumulate_grad_batches=acc, precision=precision, callbacks=list(callbacks),
                 default_root_dir="run", log_every_n_steps=1, graph_step=graph_step)
    torch.manual_seed(SEED)
    tr.fit(m, _batches(STEPS * acc))
    torch.cuda.synchronize()
    assert tr.global_step == STEPS and int(tr.optimizer._step) == STEPS
    losses = [v for _, v in tr.logged]
    params = {k: v.detach().float().cpu().clone() for k, v in m.control_model.named_parameters()}
    return tr, m, losses, params


def _assert_graph_ran(tr):
    assert tr.graph_mode == "one" and tr.graph_eager_steps <= 3
    assert tr.graph_replays == STEPS - tr.graph_eager_steps and tr.graph_replays > 0
    assert not torch.cuda.is_current_stream_capturing()


OBJECTIVE = dict(min_snr_gamma=5.0, loss_type="huber")


def _bits(precision, acc, **model):
    _, me, l_e, p_e = _fit(False, acc, precision, **model, **OBJECTIVE)
    tr, mg, l_g, p_g = _fit(True, acc, precision, **model, **OBJECTIVE)
    _assert_graph_ran(tr)
    assert me.loss_weights_pinned is False and mg.loss_weights_pinned is True
    assert len(l_e) == STEPS and len(set(l_e)) == STEPS, f"the losses must differ from step to step: {l_e}"
    print(f"[loss trainer] precision {precision} acc {acc} {model}: eager {l_e} graph {l_g}")
    assert set(p_g) == set(p_e)
    return l_e, p_e, l_g, p_g


@pytest.mark.parametrize("precision", [32, 16], ids=["fp32", "bf16"])
def test_replayed_fit_has_the_bits_of_the_eager_fit(precision):
    l_e, p_e, l_g, p_g = _bits(precision, 1)
    assert l_g == l_e, (l_g, l_e)
    diff = [k for k in p_e if not torch.equal(p_g[k], p_e[k])]
    assert not diff, f"{len(diff)} of {len(p_e)} parameters differ, e.g. {diff[:3]}"


@pytest.mark.parametrize("precision", [32, 16], ids=["fp32", "bf16"])
def test_replayed_fit_with_accumulation_has_the_bits_of_the_eager_fit(precision):
    """accumulate_grad_batches = 2, norm layers frozen (module docstring: with trainable norms no two fits share their bits)."""
    l_e, p_e, l_g, p_g = _bits(precision, 2, norm_trainable=False)
    assert l_g == l_e, (l_g, l_e)
    diff = [k for k in p_e if not torch.equal(p_g[k], p_e[k])]
    assert not diff, f"{len(diff)} of {len(p_e)} parameters differ, e.g. {diff[:3]}"


def test_replayed_fit_with_accumulation_and_trainable_norms_follows_the_eager_fit():
    """The default model at accumulate_grad_batches = 2, fp32: the same trajectory (tests/test_gpu_trainer_graph.py's gate)."""
    from tests.util import rel_l2
    l_e, p_e, l_g, p_g = _bits(32, 2)
    dl = max(abs(x - y) / abs(y) for x, y in zip(l_g, l_e))
    dp = max(rel_l2(p_g[k], p_e[k]) for k in p_e)
    print(f"[loss trainer] acc 2, trainable norms: max rel loss diff {dl:.3e}, max param rel-L2 {dp:.3e} (gates 1e-4)")
    assert dl < 1e-4 and dp < 1e-4, (dl, dp)


def test_the_objective_changes_the_trajectory():
    """The flags are not ignored: the same fit with the plain l2 loss logs other losses."""
    _, _, l_plain, _ = _fit(True)
    _, _, l_obj, _ = _fit(True, **OBJECTIVE)
    assert all(a != b for a, b in zip(l_plain, l_obj)), (l_plain, l_obj)


def test_set_loss_weights_between_replays_needs_no_new_capture():
    """After optimizer step 4 (a replay) the table is overwritten with zeros: step 5 is a replay of the same graph and logs a loss
    of exactly 0, the steps before it log the undisturbed run's losses, and the buffer did not move."""
    seen = {}

    class Swap:
        def on_train_batch_end(self, trainer, module, outputs, batch, batch_idx):
            if trainer.global_step == 4 and "ptr" not in seen:
                seen.update(ptr=module.loss_weights.data_ptr(), step=trainer._graph_step_obj, replays=trainer.graph_replays)
                assert module.loss_weights_pinned and trainer._graph_step_obj.captured
                module.set_loss_weights(torch.zeros(module.num_timesteps))
                with pytest.raises(RuntimeError, match="new capture"):
                    module.set_loss_weights(None)

    _, _, l_ref, _ = _fit(True, **OBJECTIVE)
    tr, m, l_got, _ = _fit(True, callbacks=[Swap()], **OBJECTIVE)
    _assert_graph_ran(tr)
    assert seen and seen["replays"] >= 1 and tr.graph_replays == seen["replays"] + 1, "step 5 was a replay"
    assert tr._graph_step_obj is seen["step"] and m.loss_weights.data_ptr() == seen["ptr"]
    assert l_got[:4] == l_ref[:4] and all(v > 0 for v in l_ref)
    assert l_got[4] == 0.0, l_got
