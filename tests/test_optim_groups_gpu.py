"""The grouped flat-optimizer kernels (csrc/optim.hip ``sgd_flat_groups`` / ``adam_flat_groups``) on the
GPU.  The central check needs no tolerance: the grouped op over an arena is bitwise the ungrouped
``sgd_flat`` / ``adam_flat`` called once per run on that run's slice with ``wd = run_wd`` and an lr
tensor holding the fp32 product ``lr * lr_mult`` -- a wrong run index, a table entry read out of range
or a boundary off by one vector cannot hide from it.  The arenas (``pcmp.ops.truth_optim_groups``) put
every way the lookup can go wrong on the table at the smallest size: runs of one 16-element slice,
padding inside a run, boundaries inside and exactly on a workgroup's 1024-element span, 300 runs (more
than the 256 threads that stage the table), a grid-stride loop whose second trip lies in another
run, and slices that start and end inside a run.  The fp64 truth (``torch.optim`` with ``param_groups``)
is met within ``BOUNDS`` of tests/test_optim_groups_cpu.py."""
import functools

import pytest
import torch

import pcmp  # noqa: F401
from pcmp import optim
from pcmp.ops import K, truth_optim_groups as G

from test_optim_groups_cpu import BOUNDS

pytestmark = pytest.mark.gpu
LR = 0.05


def ops():
    return torch.ops.pcmp


def _table(name, dev):
    """(run_end, run_lr_mult, run_wd, runs, arena size) of an arena on the device."""
    runs = G.runs(name)
    return (torch.tensor([e for _, e, _ in runs], dtype=torch.int64, device=dev),
            torch.tensor([G.GROUP_SETTINGS[g][0] for _, _, g in runs], dtype=torch.float32, device=dev),
            torch.tensor([G.GROUP_SETTINGS[g][1] for _, _, g in runs], dtype=torch.float32, device=dev),
            runs, G.layout(name)[1])


@functools.lru_cache(maxsize=None)
def _buffers(name, dev):
    """Random fp32 w, g and state of arena size (m2 positive), made once per arena and never written."""
    n = G.layout(name)[1]
    gen = torch.Generator(device=dev).manual_seed(7)
    w, g, m1 = (torch.randn(n, device=dev, generator=gen) for _ in range(3))
    m2 = torch.rand(n, device=dev, generator=gen) * 0.01 + 1e-4
    return w, g, m1 * 0.1, m2


def _slices(name):
    total = G.layout(name)[1]
    return [(0, total)] + (G.EDGE_SLICES if name == "edge" else [])


def _per_run(runs, lo, hi):
    for i, (s, e, _) in enumerate(runs):
        a, b = max(s, lo), min(e, hi)
        if a < b:
            yield i, a, b


# ------------------------------------------------------------------------------ bitwise: old kernels
@pytest.mark.parametrize("name", sorted(G.ARENAS))
def test_sgd_bitwise_equals_old_kernel_per_run(gpu, name):
    end, mult, wd, runs, total = _table(name, gpu)
    w0, g, m0, _ = _buffers(name, gpu)
    lr = torch.tensor([LR], device=gpu)
    big = name == "wrap"
    for lo, hi in _slices(name):
        for momentum, nesterov in ((0.9, True), (0.0, False)):
            for first in (True, False):
                for shadow in ((True,) if big else (True, False)):
                    for gs in ((0.5,) if big else (None, 0.5)):
                        gst = torch.tensor([gs], device=gpu) if gs is not None else None
                        wa, wb = w0.clone(), w0.clone()
                        ma, mb = (m0.clone(), m0.clone()) if momentum else (w0.new_empty(0), w0.new_empty(0))
                        sa = torch.full((total,), 7.0, dtype=torch.bfloat16, device=gpu) if shadow else None
                        sb = sa.clone() if shadow else None
                        ops().sgd_flat_groups(wa[lo:hi], g[lo:hi], ma[lo:hi] if momentum else ma,
                                              sa[lo:hi] if shadow else None, lr, gst, end, mult, wd, lo, total,
                                              momentum, 0.0, nesterov, first)
                        for i, a, b in _per_run(runs, lo, hi):
                            ops().sgd_flat(wb[a:b], g[a:b], mb[a:b] if momentum else mb, sb[a:b] if shadow else None,
                                           None, lr * mult[i:i + 1], gst, momentum, 0.0, float(wd[i]), nesterov, first)
                        what = (name, lo, hi, momentum, first, shadow, gs)
                        assert torch.equal(wa, wb), what
                        assert torch.equal(ma, mb), what
                        assert not shadow or torch.equal(sa, sb), what
                        assert torch.equal(wa[:lo], w0[:lo]) and torch.equal(wa[hi:], w0[hi:]), what


@pytest.mark.parametrize("name", sorted(G.ARENAS))
def test_adam_bitwise_equals_old_kernel_per_run(gpu, name):
    end, mult, wd, runs, total = _table(name, gpu)
    w0, g, m10, m20 = _buffers(name, gpu)
    lr = torch.tensor([LR], device=gpu)
    big = name == "wrap"
    for lo, hi in _slices(name):
        for decoupled in (False, True):
            for step in ((3.0,) if big else (1.0, 3.0)):
                for shadow in ((True,) if big else (True, False)):
                    for gs in ((0.5,) if big else (None, 0.5)):
                        gst = torch.tensor([gs], device=gpu) if gs is not None else None
                        st = torch.tensor([step], device=gpu)
                        a_ = [w0.clone(), m10.clone(), m20.clone()]
                        b_ = [w0.clone(), m10.clone(), m20.clone()]
                        sa = torch.full((total,), 7.0, dtype=torch.bfloat16, device=gpu) if shadow else None
                        sb = sa.clone() if shadow else None
                        ops().adam_flat_groups(a_[0][lo:hi], g[lo:hi], a_[1][lo:hi], a_[2][lo:hi],
                                               sa[lo:hi] if shadow else None, lr, gst, st, end, mult, wd, lo, total,
                                               0.9, 0.999, 1e-8, decoupled)
                        for i, a, b in _per_run(runs, lo, hi):
                            ops().adam_flat(b_[0][a:b], g[a:b], b_[1][a:b], b_[2][a:b], sb[a:b] if shadow else None,
                                            None, lr * mult[i:i + 1], gst, st, 0.9, 0.999, 1e-8, float(wd[i]), decoupled)
                        what = (name, lo, hi, decoupled, step, shadow, gs)
                        for x, y in zip(a_, b_):
                            assert torch.equal(x, y), what
                        assert not shadow or torch.equal(sa, sb), what
                        assert torch.equal(a_[0][:lo], w0[:lo]) and torch.equal(a_[0][hi:], w0[hi:]), what


@pytest.mark.parametrize("name", ["edge", "wrap"])
def test_one_run_is_bitwise_the_ungrouped_op(gpu, name):
    total = G.layout(name)[1]
    w0, g, m10, m20 = _buffers(name, gpu)
    end = torch.tensor([total], dtype=torch.int64, device=gpu)
    mult, wd = torch.ones(1, device=gpu), torch.full((1,), 0.01, device=gpu)
    lr, gst, st = torch.tensor([LR], device=gpu), torch.tensor([0.5], device=gpu), torch.tensor([2.0], device=gpu)
    wa, wb, ma, mb = w0.clone(), w0.clone(), m10.clone(), m10.clone()
    sa, sb = torch.empty(total, dtype=torch.bfloat16, device=gpu), torch.empty(total, dtype=torch.bfloat16, device=gpu)
    ops().sgd_flat_groups(wa, g, ma, sa, lr, gst, end, mult, wd, 0, total, 0.9, 0.1, False, False)
    ops().sgd_flat(wb, g, mb, sb, None, lr, gst, 0.9, 0.1, float(wd[0]), False, False)
    assert torch.equal(wa, wb) and torch.equal(ma, mb) and torch.equal(sa, sb)
    for decoupled in (False, True):
        a_, b_ = [w0.clone(), m10.clone(), m20.clone()], [w0.clone(), m10.clone(), m20.clone()]
        ops().adam_flat_groups(a_[0], g, a_[1], a_[2], sa, lr, gst, st, end, mult, wd, 0, total, 0.9, 0.999, 1e-8,
                               decoupled)
        ops().adam_flat(b_[0], g, b_[1], b_[2], sb, None, lr, gst, st, 0.9, 0.999, 1e-8, float(wd[0]), decoupled)
        for x, y in zip(a_ + [sa], b_ + [sb]):
            assert torch.equal(x, y)


# ------------------------------------------------------------------------------ truth, lr_mult 0, padding
CASES = [("sgd", v) for v in range(len(G.SGD_VARIANTS))] + [("adam", None), ("adamw", None)]


@functools.lru_cache(maxsize=None)
def _gpu_steps(kind, variant, name, gs, shadow=True):
    kw = G.SGD_VARIANTS[variant] if kind == "sgd" else G.ADAM_KW
    return G.run_steps(optim, kind, name, device="cuda", gscale=gs, shadow=shadow, **kw)[0]


@pytest.mark.parametrize("name", sorted(G.ARENAS))
def test_meets_the_fp64_truth(gpu, name):
    for kind, variant in CASES:
        kw = G.SGD_VARIANTS[variant] if kind == "sgd" else G.ADAM_KW
        for gs in ((0.5,) if name == "wrap" else (None, 0.5)):
            got = _gpu_steps(kind, variant, name, gs)
            G.check(BOUNDS, "sgd" if kind == "sgd" else "adam", name, got, G.truth_steps(kind, name, gs, **kw),
                    f"{kind} variant={variant} gscale={gs}")
            for st in got:
                assert torch.equal(st["shadow"], st["w"].to(torch.bfloat16)), "shadow == bf16(w)"
    if name == "edge":   # without the shadow: the same w and state, bitwise
        for kind, variant in CASES:
            a, b = _gpu_steps(kind, variant, name, None), _gpu_steps(kind, variant, name, None, False)
            for x, y in zip(a, b):
                assert "shadow" not in y and all(torch.equal(x[k], y[k]) for k in y)


@pytest.mark.parametrize("name", ["edge", "r300"])
def test_lr_mult_zero_keeps_w_and_padding_stays_zero(gpu, name):
    w0 = G.to_arena(name, G.case(name)["w"]).float()
    pad = G.padding_mask(name)
    for kind, variant in CASES:
        got = _gpu_steps(kind, variant, name, 0.5)
        for s, e, g in G.runs(name):
            if G.GROUP_SETTINGS[g][0] == 0.0:   # group 2: decay 0.02 and lr_mult 0 (1 - 0 * wd == 1 under AdamW)
                assert torch.equal(got[-1]["w"][s:e], w0[s:e]), (kind, s, e)
                for k in got[-1]:
                    if k not in ("w", "shadow"):
                        assert bool((got[-1][k][s:e][~pad[s:e]] != 0).all()), "the state advances"
                        assert not torch.equal(got[-1][k][s:e], got[0][k][s:e])
        for k, v in got[-1].items():
            assert int((v[pad] != 0).sum()) == 0, (kind, k, "padding stays exact zeros")


# ------------------------------------------------------------------------------ schedule, graph
def _ddp_like_buckets(name):
    """The arena cut as DistributedDataParallel cuts it: per-parameter segments, a large slice split
    into 1024-element multiples (parallel/ddp.py plan_segments), handed out last-to-first."""
    from pcmp.parallel.ddp import plan_segments
    offs, total = G.layout(name)
    sizes = [b - a for a, b in zip(offs, offs[1:] + [total])]
    return [(offs[i] + lo, offs[i] + hi) for i, lo, hi in reversed(plan_segments(sizes, 2048))]


@pytest.mark.parametrize("kind", ["sgd", "adamw"])
def test_step_equals_per_bucket_step_ranges_and_repeats_bitwise(gpu, kind):
    variant = 0 if kind == "sgd" else None
    kw = G.SGD_VARIANTS[0] if kind == "sgd" else G.ADAM_KW
    whole = _gpu_steps(kind, variant, "edge", 0.5)
    again = G.run_steps(optim, kind, "edge", device="cuda", gscale=0.5, **kw)[0]
    for a, b in zip(whole, again):
        assert all(torch.equal(a[k], b[k]) for k in a), "two runs are bitwise equal"
    buckets = _ddp_like_buckets("edge")
    assert (80, 2128) in buckets and (2128, 4176) in buckets, "the 4097-element parameter is cut inside its run"
    flat, params, groups = G.build_arena("edge", "cuda")
    opt = optim.build(kind, flat, lr=G.LR, weight_decay=G.GROUP_SETTINGS[0][1], groups=groups, **kw)
    sched = optim.LambdaLR(opt, lambda i: G.LR_FACTORS[min(i, 2)])
    opt.set_grad_scale(0.5)
    for i in range(3):
        G.set_grads(flat, params, "edge", i, "cuda")
        opt.begin_step()
        for lo, hi in buckets:
            opt.step_range(lo, hi)
        opt.end_step()
        sched.step()
        assert torch.equal(flat.master.cpu(), whole[i]["w"]) and torch.equal(flat.shadow.cpu(), whole[i]["shadow"])
        for k, v in opt._state().items():
            if k in whole[i]:
                assert torch.equal(v.cpu(), whole[i][k]), k


@pytest.mark.parametrize("kind", ["sgd", "adamw"])
def test_captured_step_replays_with_a_new_lr(gpu, kind):
    """A step captured in a torch.cuda.graph and replayed twice with lr_t changed between the replays
    equals two eager steps bitwise: the table, lr, step count and clip scale are all read on the device."""
    kw = G.SGD_VARIANTS[0] if kind == "sgd" else G.ADAM_KW
    res = []
    for graphed in (False, True):
        flat, params, groups = G.build_arena("edge", "cuda")
        opt = optim.build(kind, flat, lr=G.LR, weight_decay=G.GROUP_SETTINGS[0][1], groups=groups, **kw)
        opt.set_grad_scale(0.5)
        G.set_grads(flat, params, "edge", 0, "cuda")
        opt.step()                       # eager in both: SGD's first_step is a launch argument
        G.set_grads(flat, params, "edge", 1, "cuda")
        if graphed:
            torch.cuda.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                opt.step()
        for lr in (0.5 * G.LR, 0.25 * G.LR):
            opt.set_lr(lr)
            graph.replay() if graphed else opt.step()
        torch.cuda.synchronize()
        res.append([flat.master.clone(), flat.shadow.clone()] + [v.clone() for v in opt._state().values()])
    for a, b in zip(*res):
        assert torch.equal(a, b)


# ------------------------------------------------------------------------------ host checks
def test_host_checks(gpu):
    end, mult, wd, runs, total = _table("edge", gpu)
    w, g, m1, m2 = (t.clone() for t in _buffers("edge", gpu))
    lr, st = torch.tensor([LR], device=gpu), torch.tensor([1.0], device=gpu)

    def sgd(w_=w, g_=None, end_=end, mult_=mult, wd_=wd, base=0, arena=total, lr_=lr):
        ops().sgd_flat_groups(w_, g[:w_.numel()] if g_ is None else g_, m1[:w_.numel()], None, lr_, None, end_, mult_,
                              wd_, base, arena, 0.9, 0.0, False, False)

    def adam(w_=w, end_=end, mult_=mult, base=0, arena=total):
        ops().adam_flat_groups(w_, g[:w_.numel()], m1[:w_.numel()], m2[:w_.numel()], None, lr, None, st, end_, mult_, wd,
                               base, arena, 0.9, 0.999, 1e-8, True)

    before = w.clone()
    for fn, name in ((sgd, "sgd_flat_groups"), (adam, "adam_flat_groups")):
        with pytest.raises(RuntimeError, match=name + ": numel % 4"):
            fn(w_=w[:6])
        with pytest.raises(RuntimeError, match=name + ": base must be"):
            fn(w_=w[:8], base=2)
        with pytest.raises(RuntimeError, match=name + ": slice .* ends past the arena"):
            fn(w_=w[:8], base=total - 4)
        with pytest.raises(RuntimeError, match=name + ": the run table needs 1 to"):
            fn(end_=end[:0], mult_=mult[:0])
        with pytest.raises(RuntimeError, match=name + ": run_end, run_lr_mult and run_wd must have one length"):
            fn(mult_=mult[:-1])
        with pytest.raises(RuntimeError, match=name + ": run_end must be a contiguous int64"):
            fn(end_=end.int())
        with pytest.raises(RuntimeError, match=name + ": w must be a contiguous fp32"):
            fn(w_=w[::2][:8])
    with pytest.raises(RuntimeError, match="sgd_flat_groups: run_wd must be a contiguous fp32"):
        sgd(wd_=wd.cpu())
    with pytest.raises(RuntimeError, match="sgd_flat_groups: g must be a contiguous fp32"):
        sgd(g_=g.double())
    with pytest.raises(RuntimeError, match="sgd_flat_groups: lr must be an fp32 device scalar"):
        sgd(lr_=lr.cpu())

    # the ungrouped ops go through the same checks
    def sgd0(w_=w, m_=m1, lr_=lr, mask=None):
        ops().sgd_flat(w_, g[:w_.numel()], m_, None, mask, lr_, None, 0.9, 0.0, 0.01, False, False)

    def adam0(w_=w, m_=m1, lr_=lr, mask=None):
        ops().adam_flat(w_, g[:w_.numel()], m_, m2[:w_.numel()], None, mask, lr_, None, st, 0.9, 0.999, 1e-8, 0.01,
                        True)

    for fn, name, state in ((sgd0, "sgd_flat", "mom"), (adam0, "adam_flat", "m1")):
        with pytest.raises(RuntimeError, match=f"{name}: {state} must be a contiguous fp32"):
            fn(m_=m1[:-4])
        with pytest.raises(RuntimeError, match=name + ": w must be a contiguous fp32"):
            fn(w_=w[::2][:8], m_=m1[:8])
        with pytest.raises(RuntimeError, match=name + ": lr must be an fp32 device scalar"):
            fn(lr_=lr.cpu())
        with pytest.raises(RuntimeError, match=name + ": mask must be a contiguous uint8"):
            fn(mask=torch.ones_like(w))
        with pytest.raises(RuntimeError, match=name + ": numel % 4"):
            fn(w_=w[:6], m_=m1[:6])
    assert torch.equal(w, before), "a refused call launches nothing"


# ------------------------------------------------------------------------------ model level
def _old_kernels_per_run(opt, table):
    """``opt`` (built without groups) stepping every run of ``table`` with the ungrouped kernel: wd =
    the run's decay, lr = the fp32 product lr_t * lr_mult formed on the device."""
    runs, mult, wds, f = table.runs, table.run_lr_mult, [float(x) for x in table.run_wd.cpu()], opt.flat

    def step_range(lo, hi):
        for i, a, b in _per_run(runs, lo, hi):
            sh = f.shadow[a:b] if f.shadow is not None else None
            if isinstance(opt, optim.SGD):
                K.sgd_flat(f.master[a:b], f.grad[a:b], opt.mom[a:b] if opt.mom.numel() else opt.mom, sh, None,
                           opt.lr_t * mult[i:i + 1], opt.grad_scale, opt.momentum, opt.dampening, wds[i], opt.nesterov,
                           opt.steps == 0)
            else:
                K.adam_flat(f.master[a:b], f.grad[a:b], opt.m1[a:b], opt.m2[a:b], sh, None, opt.lr_t * mult[i:i + 1],
                            opt.grad_scale, opt.step_t, opt.beta1, opt.beta2, opt.eps, wds[i], opt.decoupled)

    opt.step_range = step_range


def _rel(a, b):
    return ((a.float() - b.float()).norm() / (b.float().norm() + 1e-12)).item()


@pytest.mark.parametrize("which", ["bert", "resnet18"])
def test_model_steps_match_per_run_old_kernels(gpu, which):
    """no_decay_1d + backbone_head_groups (four groups) on a 2-layer BERT (S = 32, B = 4, AdamW, clip 1.0,
    linear schedule) and ResNet-18 (32x32, B = 8, SGD momentum 0.9): parameters torch.equal to the
    per-run old-kernel optimizer after step 1 (same gradients) and within the bf16-noise criterion of
    tests/test_models_gpu.py (relative norm 2e-2) after 3."""
    from pcmp.engine.trainer import make_state
    from pcmp.ops import cross_entropy
    gen = torch.Generator(device=gpu).manual_seed(3)
    if which == "bert":
        from pcmp.models.bert import BertConfig, BertForSequenceClassification
        cfg = BertConfig(num_hidden_layers=2, vocab_size=2048, hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)
        ids = torch.randint(1, 2048, (4, 32), device=gpu, generator=gen)
        ids[:, 27:] = 0
        mask, y = (ids > 0).long(), torch.randint(0, 2, (4,), device=gpu, generator=gen)
        make = lambda: BertForSequenceClassification(cfg).to(gpu)             # noqa: E731
        loss_of = lambda m: m(ids, None, mask, y)[0]                          # noqa: E731
        okw, wd = dict(optimizer="adamw", lr=1e-3, eps=1e-8, clip=1.0), 0.01
    else:
        from pcmp.models.resnet import resnet18
        x = torch.rand(8, 3, 32, 32, device=gpu, generator=gen)
        y = torch.randint(0, 10, (8,), device=gpu, generator=gen)
        make = lambda: resnet18(num_classes=10).to(gpu).train()              # noqa: E731
        loss_of = lambda m: cross_entropy(m.forward_logits(x), y)             # noqa: E731
        okw, wd = dict(optimizer="sgd", lr=0.02, momentum=0.9), 5e-4
    out = []
    for grouped in (True, False):
        torch.manual_seed(11)
        m = make()
        groups = optim.compose_groups(optim.no_decay_1d(m, wd), optim.backbone_head_groups(m, 0.1))
        st = make_state(m, weight_decay=wd, groups=groups if grouped else None, **okw)
        if grouped:
            assert len(st.opt.groups.describe()) == 4 and len(st.opt.groups.runs) > 4
        else:
            assert st.opt.groups is None
            _old_kernels_per_run(st.opt, optim.ParamGroups(st.flat, groups, wd))
        st.sched = optim.linear_schedule_with_warmup(st.opt, 0, 6)
        snaps = []
        for _ in range(3):
            st.zero_grad()
            st.backward_step(loss_of(m))
            snaps.append(st.flat.master.clone())
        out.append(snaps)
    assert torch.equal(out[0][0], out[1][0]), "step 1: same gradients, bitwise the same update"
    assert not torch.equal(out[0][0], out[0][1])
    rel = _rel(out[0][2], out[1][2])
    print(which, "relative distance after 3 steps", rel)
    assert rel < 2e-2
