"""LARS / LAMB on the CPU: the reference ops of ``pcmp.ops.ref`` against the fp64 truths of
``pcmp.ops.truth_optim_layerwise`` (their floor: a tenth of the bound the kernels are held to), the ranged
step, ``state_dict`` and the ``--optimizer`` flag."""
import json

import pytest
import torch

import pcmp  # noqa: F401
from pcmp import optim
from pcmp.ops import truth_optim_layerwise as T

KINDS = ("lamb", "lars")
SHADOW_FLOOR = 0.4     # rounding w to bf16: half an ulp, 2^-9 of |w| at most, is 0.39 in norm_err's units


@pytest.mark.parametrize("name", sorted(T.ARENAS))
@pytest.mark.parametrize("kind", KINDS)
def test_reference_floor_is_a_tenth_of_the_bound(kind, name):
    for gs, degenerate in ((None, False), (0.5, name == "edge")):
        got, truth = T.run_steps(optim, kind, name, gscale=gs, degenerate=degenerate), \
            T.truth_steps(kind, name, gs, degenerate)
        T.check(name, got, truth, f"{kind} cpu gscale={gs}")
        for k, v in T.worst(name, got, truth).items():
            assert v <= (T.RATIO_RTOL if k == "ratio" else SHADOW_FLOOR if k == "shadow" else T.BOUNDS[k] / 10), (k, v)


@pytest.mark.parametrize("kind", KINDS)
def test_ranged_step_and_state_dict(kind):
    whole = T.run_steps(optim, kind, "edge", gscale=0.5)
    total = T.layout("edge")[1]
    cut = T.run_steps(optim, kind, "edge", gscale=0.5, partition=[(1600, total), (0, 1600)])
    assert all(torch.equal(a[k], b[k]) for a, b in zip(whole, cut) for k in a)
    flat, params, opt = T.build_opt(optim, kind, "many")
    flat.grad.normal_()
    opt.step()
    flat2, _, opt2 = T.build_opt(optim, kind, "many")
    opt2.load_state_dict(opt.state_dict())
    assert opt2.steps == 1 and all(torch.equal(a, b) for a, b in zip(opt._state().values(), opt2._state().values()))
    assert "trust_ratio" not in opt.state_dict()["state"]


def test_entry_point_optimizer_flag(tmp_path):
    import another_neural_net as entry
    out = tmp_path / "rec.json"
    assert entry.main(["--preset", "mlp-cpu", "--optimizer", "lamb", "--no-decay-1d", "--weight-decay", "0.01",
                       "--json", str(out)]) == 0
    rec = json.loads(out.read_text().strip().splitlines()[-1])
    assert rec["optimizer"] == "lamb" and len(rec["param_groups"]) == 2 and rec["test_loss"] == rec["test_loss"]
