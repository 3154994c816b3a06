"""``LlamaWeights.final_norm``: the raw final RMSNorm weight survives the load whether or not the norms are folded into
the projections (an embedding is pooled from the final-norm hidden state; ``norm`` itself is ones once folded)."""
import pytest
import torch

from chronos.models.llama import get_config, load_checkpoint, random_weights
from chronos.parallel.tp import TPContext

from test_checkpoint import _hf_tensors, _write_hf, _write_meta
from test_checkpoint import get_config as ckpt_config


@pytest.mark.parametrize("layout", ["hf", "meta"])
@pytest.mark.parametrize("fold", [True, False])
def test_final_norm_is_the_checkpoints(tmp_path, layout, fold):
    cfg = ckpt_config("tiny")
    t = _hf_tensors(cfg, seed=5)
    g = torch.Generator().manual_seed(0)
    t["model.norm.weight"] = (1 + torch.rand(cfg.hidden_size, generator=g) * 0.2).to(torch.bfloat16)
    (_write_hf if layout == "hf" else _write_meta)(str(tmp_path / layout), cfg, t)
    _, w = load_checkpoint(str(tmp_path / layout), fold_norms=fold)
    assert w.norms_folded == fold
    assert torch.equal(w.final_norm, t["model.norm.weight"])
    assert bool((w.norm == 1).all()) == fold
    unfolded = load_checkpoint(str(tmp_path / layout), fold_norms=False)[1]
    extra = 0 if w.final_norm is w.norm else 2 * cfg.hidden_size
    assert w.nbytes() - extra == unfolded.nbytes() - (0 if unfolded.final_norm is unfolded.norm else 2 * cfg.hidden_size)


def test_final_norm_is_replicated_under_tp(tmp_path):
    cfg = ckpt_config("tiny")
    t = _hf_tensors(cfg, seed=6)
    g = torch.Generator().manual_seed(1)
    t["model.norm.weight"] = (1 + torch.rand(cfg.hidden_size, generator=g) * 0.2).to(torch.bfloat16)
    _write_hf(str(tmp_path / "hf"), cfg, t)
    for r in range(2):
        w = load_checkpoint(str(tmp_path / "hf"), TPContext(rank=r, world=2))[1]
        assert torch.equal(w.final_norm, t["model.norm.weight"])


@pytest.mark.parametrize("fold", [True, False])
def test_random_weights_carry_final_norm(fold):
    cfg = get_config("tiny")
    w = random_weights(cfg, fold_norms=fold)
    assert w.final_norm.shape == (cfg.hidden_size,) and w.final_norm.dtype == torch.bfloat16
    assert bool((w.final_norm == 1).all())
