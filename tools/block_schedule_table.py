"""The residual-block / stem schedule as data: the op trace of one forward and backward of a fixed list
of configurations (tests/test_block_schedule_cpu.py and tests/test_block_schedule_gpu.py replay it).

Every configuration runs in a fresh child process, one after the other, with ``kernels.TRACE`` switched
on; ``params.fork_side`` / ``join_side`` / ``run_on_side`` are wrapped for the run, so the trace also
says on which stream each op was issued (``[fork_side`` ... ``]``, ``join_side``, ``[run_on_side`` ...
``]``).  A line is the op name and its arguments (a tensor as its shape), trailing ``None`` dropped;
``write_table`` stores each distinct line once and a configuration as line numbers.

    python tools/block_schedule_table.py [--out-dir tests/data]     block_schedule_{cpu,mi355x}.txt
    python tools/block_schedule_table.py --dump DIR                 also DIR/<config>.pt: loss, input
                                                                    gradient, every parameter gradient
    python tools/block_schedule_table.py --compare DIR_A DIR_B      torch.equal over two dumps
"""
import argparse
import contextlib
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SWITCHES = ("PCMP_ACT_FOLD", "PCMP_ACT_FOLD_F32", "PCMP_ACT_FOLD_MINROWS", "PCMP_DZ_FOLD", "PCMP_DZ_FOLD_MINROWS",
            "PCMP_STEM_TAIL", "PCMP_BWD_FUSED", "PCMP_STEM_S2D", "PCMP_COMPACT_DOWN", "PCMP_DOWN_STREAM",
            "PCMP_WGRAD_STREAM")
MIN0 = {"PCMP_DZ_FOLD_MINROWS": "0", "PCMP_ACT_FOLD_MINROWS": "0"}   # at these sizes no fold fires otherwise
# name -> (what to run, switches)
CONFIGS = {
    "resnet18": ("resnet18", {}),
    "resnet50": ("resnet50", {}),
    "resnet50_minrows0": ("resnet50", MIN0),
    "resnet50_minrows0_bwd_fused0": ("resnet50", {**MIN0, "PCMP_BWD_FUSED": "0"}),
    "resnet50_minrows0_dz_fold0": ("resnet50", {**MIN0, "PCMP_DZ_FOLD": "0"}),
    "resnet50_minrows0_act_fold0": ("resnet50", {**MIN0, "PCMP_ACT_FOLD": "0"}),
    "resnet50_compact_down0": ("resnet50", {"PCMP_COMPACT_DOWN": "0"}),
    "resnet50_down_stream0": ("resnet50", {"PCMP_DOWN_STREAM": "0"}),
    "resnet50_wgrad_stream0": ("resnet50", {"PCMP_WGRAD_STREAM": "0"}),
    "resnet50_stem_tail0": ("resnet50", {"PCMP_STEM_TAIL": "0"}),
    "resnet50_stem_s2d0": ("resnet50", {"PCMP_STEM_S2D": "0"}),
    "keras50": ("keras50", {}),
    "keras50_minrows0": ("keras50", MIN0),
    "resnet50_f32": ("resnet50_f32", {}),
    "resnet50_f32_act_fold": ("resnet50_f32", {"PCMP_ACT_FOLD_F32": "1"}),
    "resnet50_transfer": ("resnet50_transfer", {}),
    "bottlenecks_dx": ("bottlenecks_dx", {}),
    "bottlenecks_nodx": ("bottlenecks_nodx", {}),
    "resnet50_eval_b1": ("resnet50_eval_b1", {}),
}


def table_path(device, out_dir=os.path.join(ROOT, "tests", "data")):
    return os.path.join(out_dir, "block_schedule_%s.txt" % ("mi355x" if device.type == "cuda" else "cpu"))


def _fmt(a):
    import torch
    if isinstance(a, torch.Tensor):
        return "(" + ",".join(str(d) for d in a.shape) + ")"
    if isinstance(a, (list, tuple)):
        return "(" + ",".join(_fmt(v) for v in a) + ")"
    return repr(a)


def format_trace(trace):
    """Trace entries -> text lines; dropping trailing ``None`` arguments is the only normalisation."""
    lines = []
    for name, args in trace:
        args = list(args)
        while args and args[-1] is None:
            args.pop()
        lines.append(" ".join([name] + [_fmt(a) for a in args]))
    return lines


@contextlib.contextmanager
def side_markers():
    """Mark the side-stream calls in ``kernels.TRACE`` while the block runs."""
    from pcmp.ops import kernels, params
    saved = params.fork_side, params.join_side, params.run_on_side

    def mark(s):
        kernels.TRACE.append((s, []))

    def fork_side(fn, keep_alive):
        def inner():
            mark("[fork_side")
            try:
                return fn()
            finally:
                mark("]")
        return saved[0](inner, keep_alive)

    def join_side(*a):
        mark("join_side")
        return saved[1](*a)

    def run_on_side(fn, keep_alive, linear=False):
        def inner():
            mark("[run_on_side")
            try:
                return fn()
            finally:
                mark("]")
        return saved[2](inner, keep_alive, linear)

    params.fork_side, params.join_side, params.run_on_side = fork_side, join_side, run_on_side
    try:
        yield
    finally:
        params.fork_side, params.join_side, params.run_on_side = saved


def run(what, device):
    """One forward (and backward) of ``what`` on ``device`` under the current environment; returns the
    tensors ``--dump`` saves.  The model's parameters are flattened as in training (gradients go to
    ``main_grad``); the two chained bottlenecks keep plain autograd gradients."""
    import torch
    from pcmp.models import resnet
    from pcmp.ops import cross_entropy
    from pcmp.utils.flat import FlatParams
    torch.manual_seed(0)
    g = torch.Generator().manual_seed(1)
    if what.startswith("bottlenecks"):
        blocks = [resnet.Bottleneck(64, 64, 1).to(device).train(), resnet.Bottleneck(256, 64, 1).to(device).train()]
        x = torch.rand(4, 28, 28, 64, generator=g).to(device, torch.bfloat16).requires_grad_(what.endswith("_dx"))
        wsum = torch.rand(4, 28, 28, 256, generator=g).to(device)
        loss = (blocks[1](blocks[0](x)).float() * wsum).sum()
        loss.backward()
        ps = [p for b in blocks for p in b.parameters()]
        return {"loss": loss.detach(), "dx": x.grad, **{"grad%d" % i: p.grad for i, p in enumerate(ps)}}
    if what == "resnet50_eval_b1":
        m = resnet.resnet50(10).to(device).eval()
        with torch.no_grad():
            return {"logits": m.forward_logits(torch.rand(1, 3, 64, 64, generator=g).to(device))}
    if what == "keras50":
        m = resnet.ResNet("resnet50", 10, variant="keras")
    elif what == "resnet50_f32":
        m = resnet.resnet50(10, compute_dtype=torch.float32)
    elif what == "resnet50_transfer":
        m = resnet.resnet50_transfer(10)
    else:
        m = getattr(resnet, what)(10)
    m = m.to(device).train()
    ps = FlatParams(m.parameters()).params
    x = torch.rand(4, 3, 64, 64, generator=g).to(device)
    y = torch.randint(0, 10, (4,), generator=g).to(device)
    loss = cross_entropy(m.forward_logits(x), y)
    loss.backward()
    return {"loss": loss.detach(), **{"grad%d" % i: p.main_grad for i, p in enumerate(ps)}}


def trace_lines(name, device):
    """The trace of configuration ``name`` as text lines.  The caller has set the environment, called
    ``params.refresh_env()`` and made ``kernels.TRACE`` a list."""
    import torch
    from pcmp.ops import kernels
    from pcmp.ops.functions import dropout_rng
    del kernels.TRACE[:]
    rng = dropout_rng.seed, dropout_rng.counter
    dropout_rng.reseed(0)      # the dropout seed / offset are op arguments: as in a fresh process seeded 0
    try:
        with side_markers():
            out = run(CONFIGS[name][0], device)
    finally:
        dropout_rng.seed, dropout_rng.counter = rng
    if device.type == "cuda":
        torch.cuda.synchronize()
    return format_trace(kernels.TRACE), out


def write_table(path, traces):
    """{configuration: [lines]} as a table.  The ~6,000 trace lines are a few hundred distinct ones, so the
    file lists each distinct line once (``<number> <line>``) and gives a configuration as the numbers of its
    lines in order, or as ``== name = other`` when its trace equals an earlier configuration's."""
    number, done = {}, {}
    text = ["# tools/block_schedule_table.py: distinct trace lines, then per configuration the numbers of its lines"]
    for lines in traces.values():
        for line in lines:
            if line not in number:
                number[line] = len(number)
                text.append(f"{number[line]} {line}")
    for name, lines in traces.items():
        same = done.setdefault(tuple(lines), name)
        text.append(f"== {name}" + (f" = {same}" if same != name else ""))
        if same == name:
            nums = [str(number[line]) for line in lines]
            text += [" ".join(nums[i:i + 25]) for i in range(0, len(nums), 25)]
    with open(path, "w") as f:
        f.write("\n".join(text) + "\n")


def read_table(path):
    """{configuration: [lines]} of a table ``write_table`` wrote."""
    table, distinct, cur = {}, [], None
    with open(path) as f:
        for line in f.read().splitlines():
            if line.startswith("== "):
                name, _, same = line[3:].partition(" = ")
                cur = table[name] = list(table[same]) if same else []
            elif cur is not None:
                cur += [distinct[int(k)] for k in line.split()]
            elif line and not line.startswith("#"):
                k, _, text = line.partition(" ")
                assert int(k) == len(distinct), line
                distinct.append(text)
    return table


def child(name, out, dump):
    import torch
    import pcmp  # noqa: F401
    from pcmp.ops import _lib, kernels
    device = torch.device("cuda", 0) if torch.cuda.is_available() else torch.device("cpu")
    if device.type == "cuda":
        assert _lib.load(), _lib.load_error()
    kernels.TRACE = []
    lines, tensors = trace_lines(name, device)
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")
    if dump:
        os.makedirs(dump, exist_ok=True)
        torch.save({k: v.detach().cpu() for k, v in tensors.items() if v is not None}, os.path.join(dump, name + ".pt"))


def compare(dir_a, dir_b):
    import torch
    n = bad = 0
    for name in CONFIGS:
        a = torch.load(os.path.join(dir_a, name + ".pt"), weights_only=True)
        b = torch.load(os.path.join(dir_b, name + ".pt"), weights_only=True)
        assert a.keys() == b.keys(), name
        diff = [k for k in a if not torch.equal(a[k], b[k])]
        n += len(a)
        bad += len(diff)
        print(f"{name}: {len(a)} tensors, {len(diff)} differ")
        for k in diff:
            print(f"  {k}: max |a - b| = {(a[k].double() - b[k].double()).abs().max().item():.3e}, "
                  f"max |a| = {a[k].double().abs().max().item():.3e}")
    print(f"total: {len(CONFIGS)} configurations, {n} tensors, {bad} differ")
    return 1 if bad else 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "tests", "data"))
    ap.add_argument("--dump", default=None, metavar="DIR")
    ap.add_argument("--compare", nargs=2, default=None, metavar="DIR")
    ap.add_argument("--one", nargs=2, default=None, metavar=("CONFIG", "FILE"), help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.compare:
        sys.exit(compare(*a.compare))
    if a.one:
        return child(a.one[0], a.one[1], a.dump)
    import torch
    device = torch.device("cuda" if torch.cuda.is_available() else "cpu")   # no GPU work in this process
    path = table_path(device, a.out_dir)
    os.makedirs(a.out_dir, exist_ok=True)
    traces = {}
    for name, (_, env) in CONFIGS.items():
        e = {k: v for k, v in os.environ.items() if k not in SWITCHES and k != "PCMP_TRACE_OPS"}
        e.update(env)
        tmp = path + ".part"
        cmd = [sys.executable, os.path.abspath(__file__), "--one", name, tmp] + (["--dump", a.dump] if a.dump else [])
        subprocess.run(cmd, env=e, check=True, timeout=600)
        with open(tmp) as f:
            traces[name] = f.read().splitlines()
        os.remove(tmp)
        print(f"{name}: {len(traces[name])} trace lines", flush=True)
    write_table(path, traces)
    print("wrote", path)


if __name__ == "__main__":
    main()
