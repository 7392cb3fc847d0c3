"""Raw outputs of every conv case of ``pcmp.ops.truth_image`` on the GPU, for bitwise comparison of two
builds of the library (load another build with PCMP_LIB).

    python tools/conv_cases_dump.py OUT.pt          run every case under its knobs, save the raw outputs
    python tools/conv_cases_dump.py --compare A.pt B.pt    list the outputs that are not torch.equal

The cases and runners are the ones tests/test_image_truth_gpu.py uses (``truth_image_run``): conv_fwd
in its three forms and behind the BatchNorm-forward fold, conv_dgrad, every conv_dgrad_bnr form of a
case, conv_wgrad (the fold forms included), conv1x1_bwd_fused."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))


def dump(path):
    import pcmp  # noqa: F401
    from pcmp.ops import _lib, truth_image as T, truth_image_run as R
    from test_image_truth_cpu import bnr_forms, conv_ops
    assert _lib.load(), _lib.load_error()
    ops, dev = torch.ops.pcmp, torch.device("cuda", 0)
    out = {}

    def put(key, raw):
        for i, t in enumerate(raw):
            if t is not None:
                out[f"{key}[{i}]"] = t.detach().cpu()

    for name, case in R.all_cases().items():
        o = conv_ops(case) if name in T.CONV_CASES else ("bnr",)
        with R.knobs(ops, case["knobs"]):
            if {"fwd", "fwd_stats", "fwd_epi"} & set(o):
                put(f"{name}/fwd", R.run_conv_fwd(ops, name, dev, "fwd_epi" not in o, "fwd_stats" not in o, "fwd_res" in o)[1])
            if "dgrad" in o:
                put(f"{name}/dgrad", R.run_conv_dgrad(ops, name, dev)[1])
            if {"bnr", "bnr_halo"} & set(o):
                for form in (("recompute", "tensor") if name == "halo" else bnr_forms(name)):
                    put(f"{name}/bnr/{form}", R.run_conv_dgrad_bnr(ops, name, form, dev)[1])
            if "wgrad" in o:
                put(f"{name}/wgrad", R.run_conv_wgrad(ops, name, dev)[1])
    for name, case in T.FWD_FOLD_CASES.items():
        with R.knobs(ops, case["knobs"]):
            put(f"{name}/fwd_fold", R.run_conv_fwd_fold(ops, name, dev)[1])
    for name, case in T.WGRAD_CASES.items():
        with R.knobs(ops, case["knobs"]):
            put(f"{name}/wgrad", R.run_wgrad_case(ops, name, dev)[2])
    for M, fold in R.FUSED_SHAPES:
        put(f"fused{M}_{fold}", R.run_bwd_fused(ops, M, fold, dev)[1])
    torch.cuda.synchronize()
    torch.save(out, path)
    print(f"{len(out)} outputs of {_lib.LIB_PATH} -> {path}")


def compare(a, b):
    A, B = torch.load(a), torch.load(b)
    bad = sorted(set(A) ^ set(B))
    bad += [k for k in sorted(set(A) & set(B)) if A[k].shape != B[k].shape or not torch.equal(A[k], B[k])]
    for k in bad:
        print("DIFFERS", k)
    print(f"{len(A)} / {len(B)} outputs, {len(bad)} differ")
    return 1 if bad else 0


if __name__ == "__main__":
    if sys.argv[1] == "--compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    dump(sys.argv[1])
