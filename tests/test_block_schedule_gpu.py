"""The residual-block / stem schedule on the GPU: every configuration of tools/block_schedule_table.py
replayed in this process reproduces, line for line, the op trace recorded on an MI355X from the parent of
the change that introduced ``plan_backward`` (tests/data/block_schedule_mi355x.txt).  The trace marks the
side-stream calls, so the stream each op was issued on is part of it."""
import pytest
import torch

from test_block_schedule_cpu import replay, table

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", list(table.CONFIGS))
def test_schedule_matches_recorded_gpu(name, gpu, monkeypatch):
    lines, want = replay(name, gpu, monkeypatch)
    torch.cuda.synchronize()
    assert len(lines) == len(want)
    bad = [(i, a, b) for i, (a, b) in enumerate(zip(lines, want)) if a != b]
    assert not bad, f"{len(bad)} trace lines differ, the first: {bad[:3]}"
