"""Host side of the captured InfoNCE_dot_prod / EBM_dot_prod bucket step: the opt-in flag, and the four row-bounded entry
points in the header and in the ctypes table (their GPU tests: tests/test_gpu_contrastive_bucket.py)."""
import argparse
import os
import re

import pytest

ROWS_ENTRY_POINTS = ("msde_cl_infonce_fwd_rows", "msde_cl_infonce_bwd_rows", "msde_cl_ebm_shift_fwd_rows",
                     "msde_cl_ebm_shift_bwd_rows")


def test_captured_cl_flag_defaults_to_off():
    from moleculesde_amd import pretrain
    p = pretrain.add_hot_path_flags(argparse.ArgumentParser())
    assert p.parse_args([]).captured_cl is False
    assert p.parse_args(["--captured_cl"]).captured_cl is True
    assert pretrain.readme_args().captured_cl is False
    assert pretrain.bucket_cl_metrics(p.parse_args([])) == pretrain.BUCKET_CL_METRICS == ("EBM_node_dot_prod",)
    assert set(pretrain.bucket_cl_metrics(p.parse_args(["--captured_cl"]))) == {"EBM_node_dot_prod", "InfoNCE_dot_prod",
                                                                              "EBM_dot_prod"}
    assert pretrain.DRAWS_NEGATIVES == ("EBM_node_dot_prod",)


@pytest.mark.parametrize("name", ROWS_ENTRY_POINTS)
def test_rows_entry_point_is_declared_and_bound(name):
    """Declared in include/msde_hip.h with one parameter more than the unbounded entry point, the device count
    `const int* n_rows` in front of the stream, and listed with as many arguments in _lib.SIGNATURES."""
    from moleculesde_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "msde_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", " ", hdr, flags=re.S)

    def params(fn):
        m = re.search(r"\bint\s+%s\s*\(([^;{]*?)\)\s*;" % fn, hdr, flags=re.S)
        assert m, f"{fn} is not declared in include/msde_hip.h"
        return [" ".join(p.split()) for p in m.group(1).split(",")]
    new, old = params(name), params(name[:-len("_rows")])
    assert new[:-2] == old[:-1] and new[-2] == "const int* n_rows" and new[-1] == old[-1] == "void* stream", (new, old)
    assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name]) == len(new)
    assert _lib.SIGNATURES[name][:-2] == _lib.SIGNATURES[name[:-len("_rows")]][:-1]
    assert _lib.SIGNATURES[name][-2] is _lib.P


def test_neg_sample_check_sees_the_batch_not_the_capacity():
    from moleculesde_amd import pretrain
    from moleculesde_amd.synthetic import make_batch
    b = make_batch(2, seed=1)
    n = int(b.x.size(0))
    ok = pretrain.readme_args(CL_similarity_metric="EBM_dot_prod", CL_neg_samples=n - 1, captured_cl=True)
    pretrain.check_bucket_neg_samples(ok, b)
    with pytest.raises(ValueError, match="CL_neg_samples"):
        pretrain.check_bucket_neg_samples(pretrain.readme_args(CL_similarity_metric="EBM_dot_prod", CL_neg_samples=n,
                                                               captured_cl=True), b)
    # the other metrics have no shifts to check
    pretrain.check_bucket_neg_samples(pretrain.readme_args(CL_similarity_metric="InfoNCE_dot_prod", CL_neg_samples=n), b)
