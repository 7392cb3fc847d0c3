"""Parameter groups of the flat optimizers on the reference path: ``ops/ref.py``'s
``sgd_flat_groups`` / ``adam_flat_groups`` and ``pcmp.optim``'s ``groups=`` against ``torch.optim`` with
real ``param_groups`` (``pcmp.ops.truth_optim_groups``), the groupings of the models, the per-bucket
``step_range`` contract, the state dict and the entry-point flags.

``BOUNDS`` holds, per (optimizer, output), the worst ``norm_err`` of the reference path against the
fp64 truth over every case of tests/test_optim_groups_gpu.py (the *floor*) and the bound ``k`` the GPU
tests hold the kernels to, by the rule of tests/test_image_truth_cpu.py: a floor <= 1e-4 (fp32 state)
gets k = 0.01; every other output k = 2 * floor rounded up to a multiple of 0.5, at least 1 and
never above max(1, 4 * floor).  ``test_reference_floors`` recomputes the floors and enforces the rule.
"""
import json
import math

import pytest
import torch

import pcmp  # noqa: F401
from pcmp import optim
from pcmp.ops import truth_optim_groups as G
from pcmp.utils.flat import FlatParams

# (optimizer, output): (floor of the reference path on the CPU, bound k of the GPU tests)
BOUNDS = {
    ("sgd", "w"): (9.8e-06, 0.01), ("sgd", "mom"): (2.4e-05, 0.01), ("sgd", "shadow"): (0.256, 1.0),
    ("adam", "w"): (1.4e-05, 0.01), ("adam", "m1"): (3.4e-05, 0.01), ("adam", "m2"): (2.0e-05, 0.01),
    ("adam", "shadow"): (0.255, 1.0),
}
GS = [None, 0.5]


def measure_floors():
    fl = {}

    def upd(op, name, got, truth):
        for k, e in G.worst(name, got, truth).items():
            fl[(op, k)] = max(fl.get((op, k), 0.0), e)

    for name in G.ARENAS:
        for gs in GS:
            for v in G.SGD_VARIANTS:
                upd("sgd", name, G.run_steps(optim, "sgd", name, gscale=gs, **v)[0], G.truth_steps("sgd", name, gs, **v))
            for kind in ("adam", "adamw"):
                upd("adam", name, G.run_steps(optim, kind, name, gscale=gs, **G.ADAM_KW)[0],
                    G.truth_steps(kind, name, gs, **G.ADAM_KW))
    return fl


# ------------------------------------------------------------------------------ 1. against torch
def test_reference_floors():
    """ref against torch.optim with param_groups: SGD (momentum 0.9 with nesterov, with dampening,
    and momentum 0), Adam and AdamW, three steps with the lr changed between steps by LambdaLR."""
    fl = measure_floors()
    print({k: float("%.3g" % v) for k, v in fl.items()})
    assert set(fl) == set(BOUNDS), set(fl) ^ set(BOUNDS)
    bad = []
    for key, f in fl.items():
        rec, k = BOUNDS[key]
        if abs(f - rec) > (0.1 * rec + 0.02 if rec > 1e-4 else 0.5 * rec + 2e-6):
            bad.append((key, "floor moved", f, rec))
        want = 0.01 if rec <= 1e-4 else max(1.0, math.ceil(4 * rec) / 2)
        if k != want or (f <= 1e-4) != (rec <= 1e-4) or (f > 1e-4 and not (2 * f <= k <= max(1.0, 4 * f))):
            bad.append((key, "k must be the rule's value for the floor", f, rec, k, want))
    assert not bad, bad


def test_comparator_rejects_a_neighbours_settings():
    """One run stepped with its neighbour's decay, or a run boundary one vector late, is beyond k."""
    truth = G.truth_steps("sgd", "edge", None, **G.SGD_VARIANTS[0])
    got, _ = G.run_steps(optim, "sgd", "edge", **G.SGD_VARIANTS[0])
    G.check(BOUNDS, "sgd", "edge", got, truth)
    wrong = [dict(g) for g in got]
    # run [16, 32) (lr_mult 0.1, decay 0) updated as group 0 (lr_mult 1, decay 0.01) at step 1
    w0 = G.to_arena("edge", G.case("edge")["w"])
    g0 = G.to_arena("edge", G.case("edge")["grads"][0])
    wrong[0]["w"] = got[0]["w"].clone()
    wrong[0]["w"][16:32] = (w0 - G.LR * (g0 + 0.01 * w0))[16:32].float()
    with pytest.raises(AssertionError, match="beyond norm_err"):
        G.check(BOUNDS, "sgd", "edge", wrong, truth)
    # the boundary at 5120 one vector late: elements 5120..5123 keep group 1's update
    wrong = [dict(g) for g in got]
    wrong[0]["w"] = got[0]["w"].clone()
    wrong[0]["w"][5120:5124] = (w0 - G.LR * 0.1 * g0)[5120:5124].float()
    with pytest.raises(AssertionError, match="beyond norm_err"):
        G.check(BOUNDS, "sgd", "edge", wrong, truth)


def test_lr_mult_zero_and_padding():
    """lr_mult = 0: w keeps its bits while the state advances (AdamW with a non-zero decay too);
    alignment padding stays exact zeros in w, state and shadow after three steps."""
    for kind, kw in (("sgd", G.SGD_VARIANTS[0]), ("adam", G.ADAM_KW), ("adamw", G.ADAM_KW)):
        got, opt = G.run_steps(optim, kind, "edge", **kw)
        w0 = G.to_arena("edge", G.case("edge")["w"]).float()
        pad = G.padding_mask("edge")
        for s, e, g in G.runs("edge"):
            if G.GROUP_SETTINGS[g][0] == 0.0:
                assert torch.equal(got[-1]["w"][s:e], w0[s:e]), kind
                for k in got[-1]:
                    if k not in ("w", "shadow"):
                        assert bool((got[-1][k][s:e][~pad[s:e]] != 0).all()), (kind, k)
        for k, v in got[-1].items():
            assert int((v[pad] != 0).sum()) == 0, (kind, k)


# ------------------------------------------------------------------------------ 2. models
def _tiles(flat, runs):
    assert runs[0][0] == 0 and runs[-1][1] == flat.numel
    for (s, e, g), nxt in zip(runs, runs[1:] + [None]):
        assert s < e and s % 16 == 0 and e % 16 == 0
        if nxt is not None:
            assert e == nxt[0] and g != nxt[2], "adjacent runs are of different groups (maximal stretches)"


def _small_bert(layers=1):
    from pcmp.models.bert import BertConfig, BertForSequenceClassification
    return BertForSequenceClassification(BertConfig(num_hidden_layers=layers, vocab_size=1000, hidden_size=64,
                                                    num_attention_heads=2, intermediate_size=128,
                                                    max_position_embeddings=64))


def _ids(ps):
    return {id(p) for p in ps}


@pytest.mark.parametrize("which", ["resnet18", "bert"])
def test_no_decay_1d_selects_the_1d_parameters(which):
    from pcmp.models.resnet import resnet18
    m = resnet18(10) if which == "resnet18" else _small_bert(1)
    decay, no_decay = optim.no_decay_1d(m, 0.01)
    assert decay["weight_decay"] == 0.01 and no_decay["weight_decay"] == 0.0
    assert _ids(no_decay["params"]) == _ids(p for p in m.parameters() if p.ndim <= 1)
    assert _ids(decay["params"]) == _ids(p for p in m.parameters() if p.ndim > 1)
    picked = 0
    for n, p in m.named_parameters():   # biases, BatchNorm gammas / betas, LayerNorm gains and shifts
        leaf, owner = n.split(".")[-1], n.split(".")[-2] if "." in n else ""
        if leaf in ("bias", "gamma", "beta") or "ln" in owner:
            assert id(p) in _ids(no_decay["params"]), n
            picked += 1
    assert picked == len(no_decay["params"]) > 0
    flat = FlatParams(m.parameters(), shadow_dtype=None)
    pg = optim.ParamGroups(flat, [decay, no_decay], 0.5)
    _tiles(flat, pg.runs)
    assert len(pg.lr_mult) == 2, "every parameter is listed: no default group"
    assert sum(pg.numel) == sum(p.numel() for p in m.parameters())
    for s, e, g in pg.runs:
        inside = [p for p, o in zip(flat.params, flat.offsets) if s <= o < e]
        assert inside and all((p.ndim <= 1) == (g == 1) for p in inside)


@pytest.mark.parametrize("which", ["resnet50_transfer", "vgg16_transfer", "bert"])
def test_backbone_head_groups_selects_the_head(which):
    if which == "resnet50_transfer":
        from pcmp.models.resnet import resnet50_transfer
        m = resnet50_transfer(10)
        head = m.fc
    elif which == "vgg16_transfer":
        from pcmp.models.vgg import vgg16_transfer
        m = vgg16_transfer(10)
        head = m.classifier[-1]
    else:
        m = _small_bert(1)
        head = m.classifier
    if which != "bert":
        with pytest.raises(ValueError, match="frozen backbone"):
            optim.backbone_head_groups(m, 0.1)
        for p in m.parameters():
            p.requires_grad_(True)
    back, hd = optim.backbone_head_groups(m, 0.1)
    assert back["lr_mult"] == 0.1 and hd["lr_mult"] == 1.0
    assert _ids(hd["params"]) == _ids(head.parameters()) and len(hd["params"]) > 0
    assert _ids(back["params"]) == _ids(m.parameters()) - _ids(head.parameters())
    four = optim.compose_groups(optim.no_decay_1d(m, 0.01), [back, hd])
    assert sorted((g["lr_mult"], g["weight_decay"]) for g in four) == [(0.1, 0.0), (0.1, 0.01), (1.0, 0.0), (1.0, 0.01)]
    assert sum(len(g["params"]) for g in four) == len(list(m.parameters()))
    for g in four:
        assert all((p.ndim <= 1) == (g["weight_decay"] == 0.0) and (id(p) in _ids(head.parameters())) ==
                   (g["lr_mult"] == 1.0) for p in g["params"])
    if which != "vgg16_transfer":   # (VGG16's arena is 138 M elements: the selection is what is checked)
        flat = FlatParams(m.parameters(), shadow_dtype=None)
        pg = optim.ParamGroups(flat, four, 0.0)
        _tiles(flat, pg.runs)
        assert len(pg.lr_mult) == 4 and sum(d["runs"] for d in pg.describe()) == len(pg.runs)


def test_models_without_a_head():
    from pcmp.models.bilstm import BiLSTMClassifier
    from pcmp.models.layers import MLPHead
    for m in (BiLSTMClassifier(num_layers=1), MLPHead(16, 8, 2, 0.0)):
        with pytest.raises(ValueError, match="no distinguishable head"):
            optim.backbone_head_groups(m, 0.1)


# ------------------------------------------------------------------------------ 3. step ranges
def _partitions(name):
    total = G.layout(name)[1]
    bounds = [e for _, e, _ in G.runs(name)]
    yield [0] + bounds                                             # a cut at every run boundary
    yield [0, 1000, 3000, 5124, 5128, 6656, total]                 # cuts inside runs, one-vector slice, last run alone
    yield sorted(set([0, 4, 20, 44, 4188, 4196, 5116, total] + bounds))


@pytest.mark.parametrize("kind", ["sgd", "adamw"])
def test_step_equals_any_partition_into_step_ranges(kind):
    kw = G.SGD_VARIANTS[0] if kind == "sgd" else G.ADAM_KW
    whole, _ = G.run_steps(optim, kind, "edge", gscale=0.5, **kw)
    for cuts in _partitions("edge"):
        flat, params, groups = G.build_arena("edge")
        opt = optim.build(kind, flat, lr=G.LR, weight_decay=G.GROUP_SETTINGS[0][1], groups=groups, **kw)
        sched = optim.LambdaLR(opt, lambda i: G.LR_FACTORS[min(i, 2)])
        opt.set_grad_scale(0.5)
        for i in range(3):
            G.set_grads(flat, params, "edge", i)
            opt.begin_step()
            for lo, hi in reversed(list(zip(cuts, cuts[1:]))):   # buckets complete last-to-first
                opt.step_range(lo, hi)
            opt.end_step()
            sched.step()
            assert torch.equal(flat.master, whole[i]["w"]) and torch.equal(flat.shadow, whole[i]["shadow"]), cuts
            for k, v in opt._state().items():
                if k in whole[i]:
                    assert torch.equal(v, whole[i][k]), (k, cuts)


# ------------------------------------------------------------------------------ 4. one group
@pytest.mark.parametrize("kind", ["sgd", "adam", "adamw"])
def test_one_group_equals_the_ungrouped_optimizer(kind):
    kw = dict(G.SGD_VARIANTS[0]) if kind == "sgd" else dict(G.ADAM_KW)
    outs = []
    for grouped in (False, True):
        flat, params, _ = G.build_arena("edge")
        extra = {"groups": [{"params": list(params), "lr_mult": 1.0}]} if grouped else {}
        opt = optim.build(kind, flat, lr=G.LR, weight_decay=0.01, **kw, **extra)
        assert (opt.groups is not None) == grouped
        if grouped:
            assert len(opt.groups.runs) == 1 and opt.groups.weight_decay == [0.01]
        sched = optim.LambdaLR(opt, lambda i: G.LR_FACTORS[min(i, 2)])
        for i in range(3):
            G.set_grads(flat, params, "edge", i)
            opt.step()
            sched.step()
        outs.append([flat.master.clone(), flat.shadow.clone()] + [v.clone() for v in opt._state().values()])
    for a, b in zip(*outs):
        assert torch.equal(a, b)


# ------------------------------------------------------------------------------ 5. state dict, errors
def test_state_dict_round_trip_and_mismatch():
    flat, params, groups = G.build_arena("edge")
    opt = optim.AdamW(flat, lr=G.LR, weight_decay=0.01, groups=groups)
    G.set_grads(flat, params, "edge", 0)
    opt.step()
    sd = opt.state_dict()
    assert [g["lr_mult"] for g in sd["param_groups"]["groups"]] == [0.1, 0.0, 1.0]   # listed groups, then the default
    assert [g["weight_decay"] for g in sd["param_groups"]["groups"]] == [0.0, 0.02, 0.01]
    assert sd["param_groups"]["runs"] == [[s, e, {0: 2, 1: 0, 2: 1}[g]] for s, e, g in G.runs("edge")]
    flat2, params2, groups2 = G.build_arena("edge")
    opt2 = optim.AdamW(flat2, lr=1.0, weight_decay=0.01, groups=groups2)
    opt2.load_state_dict(sd)
    assert opt2.lr == opt.lr and opt2.steps == 1 and torch.equal(opt2.m1, opt.m1) and torch.equal(opt2.m2, opt.m2)
    # another decay, another assignment of parameters, no groups at all: each refuses the checkpoint
    groups2[0]["weight_decay"] = 0.5
    for other in (optim.AdamW(flat2, lr=1.0, weight_decay=0.01, groups=groups2),
                  optim.AdamW(flat2, lr=1.0, weight_decay=0.01, groups=[{"params": params2[:1], "lr_mult": 0.1}]),
                  optim.AdamW(flat2, lr=1.0, weight_decay=0.01)):
        with pytest.raises(ValueError, match="parameter groups differ"):
            other.load_state_dict(sd)
    # a checkpoint without groups: loads into an optimizer without groups, refused by one with
    plain = optim.AdamW(flat2, lr=0.3, weight_decay=0.01)
    psd = plain.state_dict()
    assert "param_groups" not in psd
    optim.AdamW(flat2, lr=1.0, weight_decay=0.01).load_state_dict(psd)
    with pytest.raises(ValueError, match="checkpoint without groups"):
        opt2.load_state_dict(psd)


def test_duplicate_and_foreign_parameters():
    flat, params, _ = G.build_arena("edge")
    with pytest.raises(ValueError, match="already in group 0"):
        optim.SGD(flat, groups=[{"params": params[:2]}, {"params": params[1:3]}])
    with pytest.raises(ValueError, match="not in the optimizer's arena"):
        optim.SGD(flat, groups=[{"params": [torch.nn.Parameter(torch.zeros(3))]}])
    with pytest.raises(ValueError, match="takes 'lr_mult' and 'weight_decay'"):
        optim.SGD(flat, groups=[{"params": params[:1], "lr": 0.1}])


def test_build_takes_groups():
    """Fails without the feature: ``groups=`` is a TypeError before parameter groups exist."""
    flat, params, groups = G.build_arena("edge")
    opt = optim.build("sgd", flat, lr=0.1, groups=groups)
    assert isinstance(opt.groups, optim.ParamGroups) and len(opt.groups.runs) == len(G.runs("edge"))
    assert [(s, e) for s, e, _ in opt.groups.runs] == [(s, e) for s, e, _ in G.runs("edge")]
    assert opt.groups.run_end.dtype == torch.int64 and opt.groups.run_end[-1] == flat.numel


def test_make_state_passes_groups():
    from pcmp.engine.trainer import make_state
    from pcmp.models.layers import MLPHead
    m = MLPHead(16, 8, 2, 0.0)
    st = make_state(m, "sgd", lr=0.1, weight_decay=0.01, groups=optim.no_decay_1d(m, 0.01))
    assert [d["weight_decay"] for d in st.opt.groups.describe()] == [0.01, 0.0]
    assert make_state(MLPHead(16, 8, 2, 0.0), "sgd", lr=0.1).opt.groups is None


# ------------------------------------------------------------------------------ 6. entry points
def test_entry_point_flags(tmp_path):
    import another_neural_net as entry
    out = tmp_path / "rec.json"
    assert entry.main(["--preset", "mlp-cpu", "--no-decay-1d", "--weight-decay", "0.01", "--json", str(out)]) == 0
    rec = json.loads(out.read_text().strip().splitlines()[-1])
    assert math.isfinite(rec["test_loss"])
    pg = rec["param_groups"]
    assert [(g["lr_mult"], g["weight_decay"]) for g in pg] == [(1.0, 0.01), (1.0, 0.0)]
    assert all(set(g) == {"lr_mult", "weight_decay", "numel", "runs"} and g["numel"] > 0 and g["runs"] > 0 for g in pg)
    # without the two flags no groups are built
    assert entry.main(["--preset", "mlp-cpu", "--weight-decay", "0.01", "--json", str(out)]) == 0
    assert "param_groups" not in json.loads(out.read_text().strip().splitlines()[-1])
    # a model without a distinguishable head; a transfer-learning run with a frozen backbone
    with pytest.raises(SystemExit, match=r"--backbone-lr-mult 0\.1: MLPHead has no distinguishable head"):
        entry.main(["--preset", "mlp-cpu", "--backbone-lr-mult", "0.1"])
    with pytest.raises(SystemExit, match=r"--backbone-lr-mult 0\.1: .*frozen backbone"):
        entry.main(["--device", "cpu", "--model", "resnet50", "--backbone-lr-mult", "0.1", "--train-size", "10",
                    "--image-size", "32", "--batch-size", "2"])
    assert len(out.read_text().strip().splitlines()) == 2
