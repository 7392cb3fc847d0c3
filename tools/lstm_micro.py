"""LSTM recurrence micro benchmark: lstm_seq_fwd / lstm_seq_bwd at the BiLSTM config (S=128, H=256)
per knob variant, us per call and per timestep.

  python tools/lstm_micro.py [rounds] [B] [lstm_groups values, comma separated] [H]

B = 32 (default) compares the lstm_v2 variants and prints the phase clocks.  B > 32 compares the
given lstm_groups values (default "1,0": one 32-sequence group per launch against as many as the
device holds) at the default lstm_v2, interleaved per round, and prints each one's launch plan."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import pcmp  # noqa: E402,F401
from pcmp.ops import _lib  # noqa: E402

assert _lib.load(), _lib.load_error()

ops = torch.ops.pcmp
rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 3
B = int(sys.argv[2]) if len(sys.argv) > 2 else 32
groups = [int(v) for v in sys.argv[3].split(",")] if len(sys.argv) > 3 else [1, 0]
S, H = 128, int(sys.argv[4]) if len(sys.argv) > 4 else 256
dev = torch.device("cuda")
torch.manual_seed(0)
ids = torch.randint(1, 1000, (B, S), device=dev)
for i in range(B):
    ids[i, max(1, S - (7 * i) % S):] = 0
gx = (torch.randn(B, S, 2, 4 * H, device=dev) * 0.5).to(torch.bfloat16)
whh = (torch.randn(2, 4 * H, H, device=dev) / H ** 0.5).to(torch.bfloat16)
dh = torch.randn(B, S, 2 * H, device=dev).to(torch.bfloat16)


def timeit(fn, n=20):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / n * 1e3


def check(*syncs):
    torch.cuda.synchronize()
    for s in syncs:
        assert int(s[2].item()) == 0, "barrier timeout"


h, g, c, s0 = ops.lstm_seq_fwd(gx, whh, ids)
check(s0)
print(f"B={B} S={S} H={H}: {(B + 31) // 32} groups of 32 sequences, "
      f"{torch.cuda.get_device_properties(dev).multi_processor_count} CUs", flush=True)

if B > 32 or len(sys.argv) > 3:
    for n in groups:
        ops.set_knob("lstm_groups", n)
        print(f"lstm_groups={n}: launch plan {list(ops.lstm_launch_plan(B, H))}", flush=True)
    for r in range(rounds):
        for n in groups:
            ops.set_knob("lstm_groups", n)
            check(ops.lstm_seq_fwd(gx, whh, ids)[3], ops.lstm_seq_bwd(dh, g, c, whh, ids)[1])
            tf = timeit(lambda: ops.lstm_seq_fwd(gx, whh, ids))
            tb = timeit(lambda: ops.lstm_seq_bwd(dh, g, c, whh, ids))
            print(f"round {r} B={B} lstm_groups={n}: fwd {tf:8.1f} us ({tf / S:6.2f} us/step)  "
                  f"bwd {tb:8.1f} us ({tb / S:6.2f} us/step)", flush=True)
    ops.set_knob("lstm_groups", 0)
    sys.exit(0)

for r in range(rounds):
    for v in (0, 1, 2):   # 2: v2 forward + partial-exchange backward
        ops.set_knob("lstm_v2", v)
        tf = timeit(lambda: ops.lstm_seq_fwd(gx, whh, ids))
        tb = timeit(lambda: ops.lstm_seq_bwd(dh, g, c, whh, ids))
        print(f"round {r} lstm_v2={v}: fwd {tf:7.1f} us ({tf / S:5.2f} us/step)  bwd {tb:7.1f} us ({tb / S:5.2f} us/step)",
              flush=True)

# phase clocks of workgroup 0 of group 0 (knob lstm_prof): fraction of the step per phase
ops.set_knob("lstm_prof", 1)
for v, name, fn, phases in (
        (1, "fwd", lambda: ops.lstm_seq_fwd(gx, whh, ids)[3], ["poll", "gather", "MFMA", "cell", "publish"]),
        (1, "bwd", lambda: ops.lstm_seq_bwd(dh, g, c, whh, ids)[1],
         ["cell", "publish", "poll", "A loads + MFMA", "reduce+carry"]),
        (2, "bwd v3", lambda: ops.lstm_seq_bwd(dh, g, c, whh, ids)[1],
         ["cell", "MFMA + publish", "poll", "partials gather", "carry"])):
    ops.set_knob("lstm_v2", v)
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    sync = fn()
    b.record()
    torch.cuda.synchronize()
    us = a.elapsed_time(b) * 1e3
    cyc = sync[4:20].cpu().view(torch.int64)[:len(phases)].tolist()
    tot = sum(cyc)
    print(f"{name}: {us:.1f} us, {tot / S:.0f} clocks/step over the phases; per step: " +
          ", ".join(f"{n} {v / tot * us / S:.2f} us" for n, v in zip(phases, cyc)), flush=True)
ops.set_knob("lstm_prof", 0)
ops.set_knob("lstm_v2", 2)
