"""LARS / LAMB on the GPU (csrc/optim_layerwise.hip) against the fp64 truths of
``pcmp.ops.truth_optim_layerwise``: three steps over arenas that put a one-vector segment, padding, exact
and short chunks, 300 segments and 258 partials of one segment on the table; the trust ratios within the
bound derived there; degenerate parameters at ratio exactly 1; any partition of the ranged step and a
replayed graph bitwise equal to ``step()``."""
import functools

import pytest
import torch

import pcmp  # noqa: F401
from pcmp import optim
from pcmp.ops import truth_optim_layerwise as T

pytestmark = pytest.mark.gpu
KINDS = ("lamb", "lars")


@functools.lru_cache(maxsize=None)
def _steps(kind, name, gs=None, degenerate=False, adapt_1d=False):
    return T.run_steps(optim, kind, name, "cuda", gs, degenerate, adapt_1d)


def _same(a, b):
    return all(torch.equal(x[k], y[k]) for x, y in zip(a, b) for k in x)


@pytest.mark.parametrize("name", sorted(T.ARENAS))
@pytest.mark.parametrize("kind", KINDS)
def test_meets_the_fp64_truth(gpu, kind, name):
    for gs in (None, 0.5):
        got = _steps(kind, name, gs)
        T.check(name, got, T.truth_steps(kind, name, gs), f"{kind} gscale={gs}")
        assert all(torch.equal(st["shadow"], st["w"].to(torch.bfloat16)) for st in got)


@pytest.mark.parametrize("adapt_1d", [False, True])
@pytest.mark.parametrize("kind", KINDS)
def test_degenerate_parameters_have_ratio_one(gpu, kind, adapt_1d):
    got, truth = _steps(kind, "edge", 0.5, True, adapt_1d), T.truth_steps(kind, "edge", 0.5, True, adapt_1d)
    T.check("edge", got, truth, f"{kind} degenerate adapt_1d={adapt_1d}")
    assert got[0]["ratio"][T.ZERO_W] == 1.0 and got[1]["ratio"][T.ZERO_W] != 1.0
    assert all(st["ratio"][T.ZERO_G] == 1.0 for st in got)
    assert all((st["ratio"][T.ONE_D] != 1.0) == adapt_1d for st in got)


@pytest.mark.parametrize("kind", KINDS)
def test_partitions_and_repeats_are_bitwise_step(gpu, kind):
    from pcmp.parallel.ddp import plan_segments
    whole = _steps(kind, "edge", 0.5)
    offs, total = T.layout("edge")
    ddp = [(offs[i] + lo, offs[i] + hi) for i, lo, hi in
           reversed(plan_segments([b - a for a, b in zip(offs, offs[1:] + [total])], 2048))]
    assert len(ddp) > len(offs), "a parameter is cut across buckets"
    for part in (None, ddp, [(100 * 16, total), (0, 100 * 16)]):
        assert _same(whole, T.run_steps(optim, kind, "edge", "cuda", 0.5, partition=part)), part
    flat, params, opt = T.build_opt(optim, kind, "edge", "cuda")
    opt.begin_step()
    opt.step_range(0, 64)
    with pytest.raises(RuntimeError, match="do not tile the arena"):
        opt.end_step()


@pytest.mark.parametrize("kind", KINDS)
def test_captured_step_replays_with_a_new_lr(gpu, kind):
    res = []
    for graphed in (False, True):
        flat, params, opt = T.build_opt(optim, kind, "edge", "cuda")
        opt.set_grad_scale(0.5)
        for i in range(2):
            for p, g in zip(params, T.case("edge")["grads"][i]):
                p.main_grad.copy_(g.view_as(p))
            if i == 0:
                opt.step()               # eager in both: LARS's first_step is a launch argument
        if graphed:
            torch.cuda.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                opt.step()
        for lr in (0.5 * T.LR, 0.25 * T.LR):
            opt.set_lr(lr)
            graph.replay() if graphed else opt.step()
        torch.cuda.synchronize()
        res.append([flat.master.clone(), flat.shadow.clone(), opt.trust_ratio.clone()] + list(opt._state().values()))
    assert all(torch.equal(a, b) for a, b in zip(*res))
