"""BiLSTM batches above 32 sequences on the GPU: the persistent recurrences of csrc/rnn.hip run the
32-sequence groups of a batch side by side (knob ``lstm_groups``, ``torch.ops.pcmp.lstm_launch_plan``).

Every shape of tests/test_lstm_groups_cpu.py is held to ``BOUNDS`` of the fp64 truth element-wise at
``lstm_v2`` = 0, 1 and 2, and every schedule of a batch -- all groups the device holds per launch
(``lstm_groups`` = 0), one group per launch (1), the op called on each 32-row slice -- gives the same
bits: groups are independent recurrences and the group dimension changes no arithmetic.  The sync
words are checked right after every launch, so a barrier timeout stops the test there.
"""
import functools

import pytest
import torch

import pcmp  # noqa: F401
from pcmp.ops import truth as T, truth_run as R

from test_lstm_groups_cpu import SHAPES, SHORT_SHAPES
from test_text_truth_cpu import BOUNDS

pytestmark = pytest.mark.gpu

NAMES = ("hout", "gates", "c", "dgates")


def ops():
    return torch.ops.pcmp


def _guard(sync):
    torch.cuda.synchronize()
    assert int(sync[2].item()) == 0, "barrier timeout"


class knobs:
    """Set knobs for a block, restore them after."""

    def __init__(self, **kv):
        self.kv, self.old = kv, {}

    def __enter__(self):
        for k, v in self.kv.items():
            self.old[k] = ops().set_knob(k, v)

    def __exit__(self, *exc):
        for k, v in self.old.items():
            ops().set_knob(k, v)


def _has_bwd(v, H):
    return v != 0 or H <= 384       # the round-1 backward keeps the [32][4H] dgates tile in LDS: H <= 384


@functools.lru_cache(maxsize=None)
def _case(shape):
    """(case on the GPU, fp64 truth): built once per shape, never modified."""
    dev = torch.device("cuda", 0)
    case = tuple(R.to(dev, *T.lstm_case(*shape)))
    return case, T.lstm(*case)


def _run(case, bwd=True):
    """Forward and backward on the forward's own gates / c, the sync words checked after each."""
    gx, whh, ids, dh = case
    h, g, c, sync = ops().lstm_seq_fwd(gx, whh, ids)
    _guard(sync)
    if not bwd:
        return h, g, c
    dg, sync2 = ops().lstm_seq_bwd(dh, g, c, whh, ids)
    _guard(sync2)
    return h, g, c, dg


def _run_slices(case, bwd=True):
    """The op on each 32-row slice separately (what ops/rnn.py did before the group dimension)."""
    gx, whh, ids, dh = case
    parts = [_run((gx[b0:b0 + 32].contiguous(), whh, ids[b0:b0 + 32].contiguous(), dh[b0:b0 + 32].contiguous()), bwd)
             for b0 in range(0, gx.shape[0], 32)]
    return tuple(torch.cat(ts) for ts in zip(*parts))


def _same(a, b, what):
    assert len(a) == len(b)
    for n, x, y in zip(NAMES, a, b):
        assert x.shape == y.shape and torch.equal(x, y), f"{what}: {n} differs"


@pytest.mark.parametrize("v", [2, 1, 0])
@pytest.mark.parametrize("B,S,H", SHAPES)
def test_truth(gpu, B, S, H, v):
    """Element-wise against the fp64 truth; dgates exactly 0 at padded steps, the all-pad row 2
    exactly 0 in hout and dgates.  At H = 512 lstm_v2 = 0 has a forward only, as at B <= 32."""
    case, truth = _case((B, S, H))
    ids = case[2]
    with knobs(lstm_v2=v, lstm_groups=0):
        res, raw = R.run_lstm(ops(), case, gpu, _guard, truth, _has_bwd(v, H))
    assert set(res) == set(NAMES if _has_bwd(v, H) else NAMES[:3])
    for n, e in R.worst(res).items():
        print(f"{(B, S, H)} lstm_v2={v} {n}: {e:.3f} of {BOUNDS[('lstm', n)][1]}")
    R.check(BOUNDS, "lstm", res, f"{(B, S, H)} lstm_v2={v}")
    assert float(raw[0][2].float().abs().max()) == 0.0, "hout of the all-pad row"
    if _has_bwd(v, H):
        dg, pad = raw[3], ids <= 0
        assert float(dg[pad].float().abs().max()) == 0.0, "dgates at padded steps"
        assert float(dg[2].float().abs().max()) == 0.0, "dgates of the all-pad row"


@pytest.mark.parametrize("B,S,H", SHORT_SHAPES)
def test_short_sequences(gpu, B, S, H):
    """S = 1 (no second fetch, no exchange, the loop leaves before its first wait) and S = 2 (one
    exchange, no third fetch): every lstm_v2 element-wise against the fp64 truth, and lstm_v2 = 1
    bitwise equal to lstm_v2 = 0 in every output both have (at H = 512 the forward's)."""
    case, truth = _case((B, S, H))
    raw = {}
    for v in (2, 1, 0):
        with knobs(lstm_v2=v, lstm_groups=0):
            res, raw[v] = R.run_lstm(ops(), case, gpu, _guard, truth, _has_bwd(v, H))
        assert set(res) == set(NAMES if _has_bwd(v, H) else NAMES[:3])
        for n, e in R.worst(res).items():
            print(f"{(B, S, H)} lstm_v2={v} {n}: {e:.3f} of {BOUNDS[('lstm', n)][1]}")
        R.check(BOUNDS, "lstm", res, f"{(B, S, H)} lstm_v2={v}")
    assert len(raw[0]) == (4 if _has_bwd(0, H) else 3) and len(raw[1]) == 4
    for n, a, b in zip(NAMES, raw[1], raw[0]):
        assert a.shape == b.shape and torch.equal(a, b), f"lstm_v2 = 1 against 0: {n} differs"


@pytest.mark.parametrize("v", [2, 1, 0])
@pytest.mark.parametrize("B,S,H", SHAPES)
def test_schedules_bitwise(gpu, B, S, H, v):
    """lstm_groups = 0 (automatic), 1, 1000 (every group the CUs hold) and per-slice calls agree
    bitwise in hout, gates, c and dgates; at (70, 9, 64) also lstm_groups = 2 (launches of 2 + 1
    groups); two runs at 0 agree."""
    case, _ = _case((B, S, H))
    bwd = _has_bwd(v, H)
    with knobs(lstm_v2=v, lstm_groups=0):
        base = _run(case, bwd)
        again = _run(case, bwd)
        ops().set_knob("lstm_groups", 1)
        assert set(ops().lstm_launch_plan(B, H)) == {1}
        one = _run(case, bwd)
        slices = _run_slices(case, bwd)
        ops().set_knob("lstm_groups", 1000)           # as many groups as the CUs hold: one launch of 8 + 1 at (257, 3, 256)
        _same(base, _run(case, bwd), "lstm_groups = 1000")
        if (B, S, H) == (70, 9, 64):
            ops().set_knob("lstm_groups", 2)
            assert list(ops().lstm_launch_plan(B, H)) == [2, 1]
            _same(base, _run(case, bwd), "lstm_groups = 2")
    _same(base, again, "second run at lstm_groups = 0")
    _same(base, one, "lstm_groups = 1")
    _same(base, slices, "per-slice calls")


def _rule(B, H, cus, knob):
    """The documented plan: at most G_max = floor(CUs / (2 * H / 16)) groups of 32 sequences per
    launch (one workgroup per CU); the automatic count (knob 0) is the measured best: half the CUs,
    all of them at H <= 64."""
    wgs = 2 * (H // 16)
    ng, gmax = -(-B // 32), max(1, cus // wgs)
    G = min(knob, gmax) if knob > 0 else (gmax if H <= 64 else max(1, (cus // 2) // wgs))
    return [min(G, ng - g0) for g0 in range(0, ng, G)]


def test_launch_plan(gpu):
    cus = torch.cuda.get_device_properties(gpu).multi_processor_count
    shapes = [(B, H) for B, _, H in SHAPES] + [(1, 256), (32, 256), (256, 256), (512, 256), (300, 512), (1000, 64)]
    with knobs(lstm_groups=0):
        for knob in (0, 1, 2, 3, 1000):
            ops().set_knob("lstm_groups", knob)
            for B, H in shapes:
                plan = list(ops().lstm_launch_plan(B, H))
                assert plan == _rule(B, H, cus, knob), (B, H, knob, plan)
                assert sum(plan) == -(-B // 32) and max(plan) * 2 * (H // 16) <= max(cus, 2 * (H // 16))
                if knob == 1:
                    assert set(plan) == {1}
        if cus == 256:
            ops().set_knob("lstm_groups", 1000)       # the residency limit G_max: 8 at H = 256, 4 at H = 512
            assert list(ops().lstm_launch_plan(257, 256)) == [8, 1]
            assert list(ops().lstm_launch_plan(40, 512)) == [2]
            assert list(ops().lstm_launch_plan(1000, 512)) == [4] * 8
            ops().set_knob("lstm_groups", 0)          # automatic: capped at the measured best
            assert list(ops().lstm_launch_plan(257, 256)) == [4, 4, 1]
            assert list(ops().lstm_launch_plan(40, 512)) == [2]
            assert list(ops().lstm_launch_plan(1000, 512)) == [2] * 16
            assert list(ops().lstm_launch_plan(1025, 64)) == [32, 1]


@pytest.mark.parametrize("v", [2, 1])
def test_groups_are_isolated(gpu, v):
    """Other inputs in the rows of group 1 leave groups 0 and 2 bitwise unchanged, forward and
    backward (and do change group 1)."""
    case, _ = _case((70, 9, 64))
    gx, whh, ids, dh = (t.clone() for t in case)
    gen = torch.Generator().manual_seed(5)
    gx[32:64] = (torch.randn(32, *gx.shape[1:], generator=gen) * 0.5).to(gx.dtype).to(gpu)
    ids[32:64] = torch.randint(0, 3, (32, ids.shape[1]), generator=gen).to(gpu)
    dh[32:64] = torch.randn(32, *dh.shape[1:], generator=gen).to(dh.dtype).to(gpu)
    with knobs(lstm_v2=v, lstm_groups=0):
        assert sum(ops().lstm_launch_plan(70, 64)) == 3
        base = _run(case)
        other = _run((gx, whh, ids, dh))
    for n, a, b in zip(NAMES, base, other):
        assert torch.equal(a[:32], b[:32]) and torch.equal(a[64:], b[64:]), f"{n}: group 0 / 2 changed"
        assert not torch.equal(a[32:64], b[32:64]), f"{n}: group 1 did not change"


@pytest.mark.parametrize("B", [40, 24])
def test_model_bitwise_across_lstm_groups(gpu, B):
    """BiLSTMClassifier(vocab 1000, embed 64, hidden 64, 2 layers), S = 12, no dropout: the loss and
    every gradient are bitwise equal between lstm_groups = 1 and 0, and finite."""
    from pcmp.models.bilstm import BiLSTMClassifier
    from pcmp.ops import cross_entropy
    from pcmp.ops.rnn import check_errors
    torch.manual_seed(0)
    m = BiLSTMClassifier(1000, 64, 64, 2, 2, 0.0).to(gpu).train()
    gen = torch.Generator().manual_seed(B)
    ids = T.lstm_ids(B, 12, gen).to(gpu)
    y = torch.randint(0, 2, (B,), generator=gen).to(gpu)

    def grads():
        for p in m.parameters():
            p.grad = None
        loss = cross_entropy(m.forward_logits(ids), y)
        loss.backward()
        check_errors()
        return loss.detach().clone(), {n: p.grad.clone() for n, p in m.named_parameters()}

    with knobs(lstm_groups=1):
        grads()                               # the first call of a shape tunes its WGRAD split counts
        l1, g1 = grads()
        ops().set_knob("lstm_groups", 0)
        l0, g0 = grads()
    assert torch.isfinite(l0) and torch.equal(l0, l1)
    assert set(g0) == set(g1) == {n for n, _ in m.named_parameters()}
    for n in g0:
        assert torch.isfinite(g0[n]).all() and torch.equal(g0[n], g1[n]), n


def test_sync_words_with_phase_clocks(gpu):
    """With lstm_prof the counters of groups 1, 2, ... sit behind the 16 profile words: 4 + 16 + 2 * 2
    words for three groups, the same bits as without, and only group 0 writes clocks."""
    case, _ = _case((70, 9, 64))
    gx, whh, ids, dh = case
    with knobs(lstm_v2=2, lstm_groups=0, lstm_prof=0):
        base = _run(case)
        assert ops().lstm_seq_fwd(gx, whh, ids)[3].numel() == 4 + 2 * 2
        ops().set_knob("lstm_prof", 1)
        h, g, c, sync = ops().lstm_seq_fwd(gx, whh, ids)
        _guard(sync)
        dg, sync2 = ops().lstm_seq_bwd(dh, g, c, whh, ids)
        _guard(sync2)
    _same(base, (h, g, c, dg), "lstm_prof = 1")
    S, nub = 9, 64 // 16
    for s in (sync, sync2):
        assert s.numel() == 4 + 16 + 2 * 2
        w = s.cpu().tolist()
        # every counter pair counted (S - 1) hand-offs of nub workgroups per direction
        assert w[0] == w[1] == w[20] == w[21] == w[22] == w[23] == (S - 1) * nub, w
        assert w[2] == 0 and w[3] == 0
        assert sum(s[4:20].cpu().view(torch.int64)[:5].tolist()) > 0


def test_refusals(gpu):
    """The hidden-size check is unchanged; a batch of 33 is no longer refused."""
    gx, whh, ids, dh = (t.to(gpu) for t in T.lstm_case(3, 4, 48))
    with pytest.raises(RuntimeError, match="hidden size must be a multiple of 32, <= 512"):
        ops().lstm_seq_fwd(gx, whh, ids)
    with pytest.raises(RuntimeError, match="hidden size must be a multiple of 32, <= 512"):
        ops().lstm_launch_plan(3, 48)
    case, _ = _case((33, 5, 64))
    h, g, c, dg = _run(case)
    assert h.shape == (33, 5, 128) and dg.shape == (33, 5, 2, 256)
