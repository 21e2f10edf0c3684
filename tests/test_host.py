"""CPU tests of host logic and the C-ABI boundary (library loads, exports every symbol
include/recsys_hip.h declares, rejects bad arguments without touching a GPU)."""
import ctypes as C

import numpy as np
import pytest

from recommender_amd import _lib as L


def test_library_exports_header_symbols(lib):
    syms = L.header_symbols()
    assert len(syms) >= 15
    missing = [s for s in syms if not hasattr(lib, s)]
    assert not missing, missing
    assert lib.rs_version() >= 1


def test_every_header_symbol_has_a_python_signature():
    assert set(L.header_symbols()) <= set(L.SIGNATURES)


_I32, _I64, _P, _SZ = C.c_int32, C.c_int64, C.c_void_p, C.c_size_t

SYNTHETIC_HEADER = """
/* a comment with a declaration in it: int32_t rs_fake(int x); */
#ifndef SYNTHETIC_H
#define SYNTHETIC_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif
#define RS_THREE 3
#define RS_MINUS_TWO (-2) /* parenthesised */
#define RS_HEX 0x10       // sixteen; int32_t rs_fake(int x);
#define RS_NOT_A_NUMBER "text"
typedef struct rs_some_point {
  float x, y, z; /* a run */
  const int32_t* idx;
  float* rows[3];
  int64_t n;
} rs_some_point;
// int32_t rs_fake(int x);
const char* rs_name(void);
void* rs_make(void);
size_t rs_size(int64_t n, int32_t d);
int32_t rs_go(const float* a, float const* b, uint32_t k, uint64_t seed, float eps,
              const rs_some_point* p, const float* const* many, void* stream);
#ifdef __cplusplus
}
#endif
#endif /* SYNTHETIC_H */
"""


def test_header_reader_on_a_synthetic_header():
    from recommender_amd._header import read_header

    consts, structs, funcs = read_header(SYNTHETIC_HEADER)
    assert consts == {"RS_THREE": 3, "RS_MINUS_TWO": -2, "RS_HEX": 16}
    assert list(structs) == ["rs_some_point"]
    pt = structs["rs_some_point"]
    assert pt.__name__ == "SomePoint" and issubclass(pt, C.Structure)
    assert pt._fields_ == [("x", C.c_float), ("y", C.c_float), ("z", C.c_float), ("idx", _P),
                           ("rows", _P * 3), ("n", _I64)]
    assert funcs == {
        "rs_name": (C.c_char_p, []),
        "rs_make": (_P, []),
        "rs_size": (_SZ, [_I64, _I32]),
        "rs_go": (_I32, [_P, _P, C.c_uint32, C.c_uint64, C.c_float, C.POINTER(pt), _P, _P]),
    }
    assert list(funcs) == ["rs_name", "rs_make", "rs_size", "rs_go"]


@pytest.mark.parametrize("decl, named", [
    ("int32_t rs_bad_param(const float* a, double x);", "rs_bad_param"),
    ("void rs_bad_return(void);", "rs_bad_return"),
    ("int32_t rs_by_value(rs_some_point p);", "rs_by_value"),
    ("int32_t rs_unnamed(int32_t, float);", "rs_unnamed"),
    ("typedef struct rs_bad_struct { double d; } rs_bad_struct;", "rs_bad_struct"),
])
def test_header_reader_refuses_what_it_cannot_type(decl, named):
    from recommender_amd._header import read_header

    text = SYNTHETIC_HEADER.replace("const char* rs_name(void);", decl)
    with pytest.raises(ValueError, match=named):
        read_header(text)


def test_header_reader_on_the_real_header():
    import re

    F = C.c_float
    assert len(L.SIGNATURES) >= 170
    # the names, by the plain regex the binding used before it read whole declarations
    text = L.HEADER.read_text()
    names = set(re.findall(r"^\s*(?:const\s+)?[\w\s\*]+?\b(rs_\w+)\s*\(", text, re.M))
    assert set(L.header_symbols()) == names == set(L.SIGNATURES)
    assert L.header_symbols() == sorted(names)
    assert L.SIGNATURES["rs_embedding_fwd"] == (
        _I32, [_P, _I64, _I32, _P, _I32, _I64, _P, _I32, _P, _P, _P])
    assert L.SIGNATURES["rs_bce_fwd"] == (_I32, [_P, _P, _I64, F, _I32, _P, _P, _SZ, _P])
    assert L.SIGNATURES["rs_dlrm_dense_tail"] == (_I32, [C.POINTER(L.DlrmTailArgs), _P, _SZ, _P])
    assert L.SIGNATURES["rs_last_error"] == (C.c_char_p, [])
    assert L.SIGNATURES["rs_event_create"] == (_P, [])
    assert L.SIGNATURES["rs_keras_adam_flat"][1][7] is C.POINTER(L.AdamParams)


def test_load_sets_the_header_signatures(lib):
    for name, (res, args) in L.SIGNATURES.items():
        f = getattr(lib, name)
        assert f.restype is res and list(f.argtypes) == args, name


def test_struct_layout_matches_the_host_compiler(tmp_path):
    """sizeof and every offsetof of the two argument structs, as g++ (the host compiler of
    recommender_amd/build.py) lays them out from the header, against the generated ctypes."""
    import subprocess

    structs = {"rs_adam_params": L.AdamParams, "rs_dlrm_tail_args": L.DlrmTailArgs}
    assert [f[0] for f in L.AdamParams._fields_] == ["lr", "beta1", "beta2", "one_minus_beta1",
                                                     "one_minus_beta2", "epsilon"]
    assert len(L.DlrmTailArgs._fields_) == 29 and L.DlrmTailArgs._fields_[-1] == ("lr", C.c_float)
    lines = ["#include <cstddef>", "#include <cstdio>", '#include "recsys_hip.h"', "int main() {"]
    for cname, cls in structs.items():
        lines.append(f'  std::printf("{cname} sizeof %zu\\n", sizeof({cname}));')
        lines += [f'  std::printf("{cname} {n} %zu\\n", offsetof({cname}, {n}));'
                  for n, _ in cls._fields_]
    src, exe = tmp_path / "layout.cpp", tmp_path / "layout"
    src.write_text("\n".join(lines + ["  return 0;", "}"]) + "\n")
    subprocess.run(["g++", "-std=c++17", f"-I{L.HEADER.parent}", str(src), "-o", str(exe)],
                   check=True, capture_output=True, text=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout
    got = [tuple(line.split()) for line in out.splitlines()]
    want = []
    for cname, cls in structs.items():
        want.append((cname, "sizeof", str(C.sizeof(cls))))
        want += [(cname, n, str(getattr(cls, n).offset)) for n, _ in cls._fields_]
    assert got == want
    prm = L.AdamParams(1e-3, 0.9, 0.999, 0.1, 0.001, 1e-7)  # positional, as bench.py builds it
    assert (prm.lr, prm.epsilon) == (C.c_float(1e-3).value, C.c_float(1e-7).value)


def test_header_constants_are_module_attributes():
    import re

    defs = re.findall(r"^#define\s+(RS_\w+)\s+\(?(-?\d+)\)?", L.HEADER.read_text(), re.M)
    assert len(defs) >= 18
    for name, value in defs:
        assert getattr(L, name) == int(value), name
    assert (L.RS_ID_I32, L.RS_ID_I64, L.RS_DEDUP_TILE, L.RS_DIEN_SKIP_MASKED_ROWS) == (0, 1, 32, 1)
    assert (L.RS_OPT_SGD, L.RS_OPT_LAZY_ADAM, L.RS_OPT_KERAS_ADAM) == (0, 1, 2)
    assert (L.RS_ERRBIT_OOB, L.RS_ERRBIT_FORMAT, L.RS_ERRBIT_RANGE) == (1, 2, 4)
    assert L.RS_E_INVALID == -1 and L.RS_E_UNSUPPORTED == -5


def test_workspace_buffers_on_cpu_tensors():
    import torch

    cpu, meta = torch.device("cpu"), torch.device("meta")
    ws = L.Workspace()
    a = ws.get("a", 1000, cpu)
    assert a.dtype == torch.uint8 and a.numel() == 1000 and a.device == cpu
    assert ws.get("a", 10, cpu) is a and ws.get("a", 1000, cpu) is a  # smaller or equal: reused
    big = ws.get("a", 1001, cpu)
    assert big is not a and big.numel() == 1001 and ws.get("a", 1000, cpu) is big  # grow-only
    assert ws.get("small", 1, cpu).numel() == 256  # the floor
    b = ws.get("b", 1001, cpu)
    assert b.data_ptr() != big.data_ptr() and ws.get("a", 1, cpu) is big  # names never alias
    other = ws.get("a", 8, meta)
    assert other.device == meta and other is not big  # another device: a new buffer
    assert L.Workspace().get("a", 1001, cpu).data_ptr() != big.data_ptr()  # nor do two owners
    # the process-wide buffers: one per (name, device)
    s = L.workspace("test_host.x", 300, cpu)
    assert L.workspace("test_host.x", 200, cpu) is s
    assert L.workspace("test_host.y", 300, cpu).data_ptr() != s.data_ptr()
    assert L.workspace("test_host.x", 300, meta).device == meta
    assert L.workspace("test_host.x", 300, cpu) is s  # the other device did not displace it
    # a fresh buffer of exactly the bytes asked for, at least one
    f = L.scratch(10, cpu)
    assert f.dtype == torch.uint8 and f.numel() == 10 and L.scratch(0, cpu).numel() == 1
    assert L.scratch(10, cpu).data_ptr() != f.data_ptr()


def test_build_id_matches_sources_and_stale_library_is_refused(lib):
    from recommender_amd.build import source_hash

    assert lib.rs_build_id().decode() == source_hash()

    class Stale:
        @staticmethod
        def rs_build_id():
            return b"0000000000000000"

    with pytest.raises(L.RecsysError, match="other sources"):
        L.check_build_id(Stale(), "stale.so")


def test_argument_validation_without_gpu(lib):
    # null table with n_ids > 0 → RS_E_INVALID and a message, no device access
    st = lib.rs_embedding_fwd(None, 10, 4, None, 1, 5, None, 1, None, None, None)
    assert st == -1
    assert b"null" in lib.rs_last_error()
    assert lib.rs_embedding_fwd(None, 10, 0, None, 1, 5, None, 1, None, None, None) == -1
    assert lib.rs_dot_interaction_fwd(None, 4, 3, 8, 0, 1, None, 2, None) == -1  # stride < F*F
    with pytest.raises(L.RecsysError):
        L.check(-1, "rs_x")


def test_workspace_queries(lib):
    assert lib.rs_sort_ids_workspace_size(1 << 20) > 8 << 20
    assert lib.rs_apply_workspace_size(1 << 20, 128) >= (1 << 20) // 32 * 2 * 128 * 4


def test_no_cpu_fallback():
    import torch

    from recommender_amd.functional import dot_interaction

    with pytest.raises(L.RecsysError):
        dot_interaction(torch.zeros(2, 3, 4), False, True)


def test_dlrm_scheduler_matches_reference_formula():
    from recommender_amd.optim import DLRMScheduler

    s = DLRMScheduler(0.01, 20, 10000, 0.0001)
    assert s(0) == 0.0
    assert abs(s(10) - 0.005) < 1e-9
    assert abs(s(20) - 0.01) < 1e-9
    mid = s(20 + 5000)
    assert abs(mid - 0.01 * ((1 - 1e-4) * 0.5 * (1 + np.cos(np.pi * 0.5)) + 1e-4)) < 1e-7
    assert abs(s(10 ** 6) - 0.01 * 1e-4) < 1e-9


def test_keras_adam_coefficients_host():
    from oracle.embedding import keras_adam_coefficients as ref
    from recommender_amd.optim import keras_adam_coefficients

    for t in (1, 7, 100):
        assert np.float32(keras_adam_coefficients(t).lr) == ref(t)["lr"]


def test_criteo_cardinalities_and_ids():
    from recommender_amd.synthetic import criteo_batch, criteo_cardinalities

    c = criteo_cardinalities()
    assert len(c) == 26 and sum(c) == 40_000_000
    rng = np.random.default_rng(4)
    cat, dn, lb = criteo_batch(rng, 4096, c)
    assert cat.shape == (4096, 26) and (cat >= 0).all() and (cat < np.array(c)).all()
    assert dn.shape == (4096, 13) and abs(lb.mean() - 0.256) < 0.03


def test_graph_keras_adam_flat_layout_cpu():
    """GraphKerasAdam's flat buffers (host logic only, no kernel call): every parameter becomes a
    16-byte-aligned view of `flat` with its values kept, and grad_view(i) is the same slice of
    `grad_flat`, so a densified gradient written there lands where rs_keras_adam_flat reads it
    and the padding between parameters stays 0."""
    import torch

    from recommender_amd.optim import GraphKerasAdam

    ps = [torch.nn.Parameter(torch.arange(n, dtype=torch.float32).reshape(shape))
          for n, shape in ((6, (2, 3)), (5, (5,)), (8, (4, 2)))]
    want = [p.detach().clone() for p in ps]
    opt = GraphKerasAdam(ps, lr=1e-3, window=4)
    for i, (p, w) in enumerate(zip(ps, want)):
        assert torch.equal(p.detach(), w)
        o, n, pad = opt._segs[i]
        assert o % 4 == 0 and (n + pad) % 4 == 0
        assert p.data_ptr() == opt.flat[o:].data_ptr()
        gv = opt.grad_view(i)
        assert gv.shape == p.shape and gv.data_ptr() == opt.grad_flat[o:].data_ptr()
        gv.fill_(float(i + 1))
    pad_mask = torch.ones_like(opt.grad_flat, dtype=torch.bool)
    for i, (o, n, _) in enumerate(opt._segs):
        assert torch.all(opt.grad_flat[o:o + n] == float(i + 1))
        pad_mask[o:o + n] = False
    assert torch.all(opt.grad_flat[pad_mask] == 0)


def test_bench_plain_run_is_the_default_and_full_is_opt_in(monkeypatch):
    import sys

    import bench

    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "2"])
    a = bench.parse()
    assert (a.full, a.dump_outputs, a.steps, a.warmup) == (False, None, 7, 2)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "d"])
    a = bench.parse()
    assert a.full is True and a.dump_outputs == "d"


def test_bench_dump_outputs_files_budget_and_repeatability(tmp_path, monkeypatch):
    """bench.py --dump-outputs on host tensors: float32 / float64 .npy files of the loss, the
    predictions, every parameter and the batch's table rows; an array over its budget is cut to
    the same seeded sample on every call."""
    import argparse
    import os

    import torch

    import bench

    monkeypatch.setattr(bench, "DUMP_ARRAY_BYTES", 4 * 100)
    monkeypatch.setattr(bench, "DUMP_TABLE_BYTES", 4 * 8 * 5)
    g = torch.Generator().manual_seed(4)
    model = torch.nn.Module()
    model.lin = torch.nn.Linear(30, 20)  # weight: 600 elements, over the 100-element budget
    model.embedding_layer = torch.nn.Module()
    model.embedding_layer.grad_handle = torch.nn.Parameter(torch.zeros(0))
    model.embedding_layer.register_buffer("weight", torch.rand(40, 8, generator=g))
    model.embedding_layer.register_buffer("slot_offsets", torch.tensor([0, 10, 40]))
    step = argparse.Namespace(last_pred=torch.rand(16, generator=g))
    cat = torch.stack([torch.randint(0, 10, (16,), generator=g),
                       torch.randint(0, 30, (16,), generator=g)], 1)
    args = argparse.Namespace(seed=4)
    got = []
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), args, model, step, torch.tensor(0.5), (cat, None, None))
        got.append({f: np.load(tmp_path / d / f) for f in sorted(os.listdir(tmp_path / d))})
    a, b = got
    assert set(a) == {"loss.npy", "predictions.npy", "param.lin.weight.npy", "param.lin.bias.npy",
                      "embedding_row_ids.npy", "embedding_rows.npy"}
    for f in a:
        assert a[f].dtype == (np.float64 if f == "embedding_row_ids.npy" else np.float32), f
        np.testing.assert_array_equal(a[f], b[f])
    assert a["loss.npy"].tolist() == [0.5]
    np.testing.assert_array_equal(a["predictions.npy"], step.last_pred.numpy())
    np.testing.assert_array_equal(a["param.lin.bias.npy"], model.lin.bias.detach().numpy())
    w = model.lin.weight.detach().numpy().reshape(-1)
    assert a["param.lin.weight.npy"].shape == (100,) and np.isin(a["param.lin.weight.npy"], w).all()
    rows = a["embedding_row_ids.npy"].astype(np.int64)
    touched = np.unique(cat.numpy() + np.array([0, 10]))
    assert rows.shape == (5,) and (np.diff(rows) > 0).all() and np.isin(rows, touched).all()
    np.testing.assert_array_equal(a["embedding_rows.npy"], model.embedding_layer.weight.numpy()[rows])


def test_bench_pmc_filter_keeps_every_family_main_kernel():
    """bench.py's PMC passes filter kernels by PMC_KERNEL_REGEX and count each family's calls by
    its main kernel: a main kernel the filter drops leaves the family at 0 calls and the line's
    traffic null (a round-5 regression: the slot-segmented sort's kernels were filtered out)."""
    import re

    import bench

    for entry, _, main in bench.PMC_SYMBOLS:
        for alt in main.split("|"):
            name = "void rs::" + re.sub(r"\\d\+", "9", alt).replace("\\", "") + "(...)"
            assert re.search(bench.PMC_KERNEL_REGEX, name), (entry, alt)
