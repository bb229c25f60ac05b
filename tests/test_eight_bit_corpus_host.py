"""The C ABI of the rerank on an 8-bit corpus (lshrs_cosine_{batch,ragged}_{i8,f8e4m3}) and of the row quantizer
(lshrs_quantize_rows_{i8,f8e4m3}): declared in include/lshrs_hip.h, bound in lshrs_amd/_native.py, exported by the library,
and checking their arguments before anything touches a device.  CPU only - no kernel is launched here."""

from __future__ import annotations

import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "lshrs_hip.h")
COSINE = {"lshrs_cosine_batch_i8": "const int8_t", "lshrs_cosine_ragged_i8": "const int8_t",
          "lshrs_cosine_batch_f8e4m3": "const uint8_t", "lshrs_cosine_ragged_f8e4m3": "const uint8_t"}
QUANT = {"lshrs_quantize_rows_i8": "int8_t", "lshrs_quantize_rows_f8e4m3": "uint8_t"}
BADARG, TOOLARGE = -10001, -10002


@pytest.fixture(scope="module")
def lib():
    from lshrs_amd import _native

    _native.build()
    return _native.load()


def _header_text():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def _exported():
    from lshrs_amd import _native

    out = subprocess.run(["nm", "-D", "--defined-only", _native.LIBRARY], capture_output=True, text=True, check=True)
    return {line.split()[-1] for line in out.stdout.splitlines() if " T " in line}


def test_the_six_entries_are_declared_bound_and_exported(lib):
    from lshrs_amd import _native

    text, exported = _header_text(), _exported()
    for name, ctype in COSINE.items():
        assert re.search(r"\bint\s+" + name + r"\s*\(\s*" + ctype + r"\* corpus,", text), name
        assert name in _native.EXPORTS and name in exported, name
        f32 = name.rsplit("_", 1)[0] + "_f32"
        assert getattr(lib, name).argtypes == getattr(lib, f32).argtypes, name      # the f32 entry's signature
    for name, ctype in QUANT.items():
        assert re.search(r"\bint\s+" + name + r"\s*\(\s*const float\* X, int64_t n, int64_t ldx, int32_t dim, " + ctype
                         + r"\* out, int64_t ldo,\s*uint8_t\* status,\s*void\* stream\)", text), name
        assert name in _native.EXPORTS and name in exported, name
        assert len(getattr(lib, name).argtypes) == 8, name
    assert lib.lshrs_abi_version() == 7                                             # additive: the ABI number stays


def test_batch_entries_check_their_arguments_without_a_device(lib):
    buf = 0x1000                   # (never dereferenced: every call below returns before a launch)
    for name in ("lshrs_cosine_batch_i8", "lshrs_cosine_batch_f8e4m3"):
        fn = getattr(lib, name)
        # (corpus, m, ldc, dim, queries, q, cand_idx, c, scores, status, qstatus, stream)
        assert fn(None, 10, 8, 8, buf, 1, buf, 3, buf, buf, buf, None) == BADARG, name          # null corpus
        assert fn(buf, 10, 7, 8, buf, 1, buf, 3, buf, buf, buf, None) == BADARG, name           # ldc < dim (elements)
        assert fn(buf, 10, 8, 8, None, 1, buf, 3, buf, buf, buf, None) == BADARG, name          # null queries
        assert fn(buf, 10, 8, 8, buf, 1, buf, 3, None, buf, buf, None) == BADARG, name          # null scores
        assert fn(buf, 10, 8, 8, buf, 4, None, 3, buf, buf, buf, None) == BADARG, name          # dense candidates past m
        assert fn(buf, 10, 16385, 16385, buf, 1, buf, 3, buf, buf, buf, None) == TOOLARGE, name
        assert fn(None, 10, 8, 8, None, 0, None, 3, None, None, None, None) == 0, name          # q == 0: nothing to do
        assert fn(None, 10, 8, 8, None, 2, None, 0, None, None, None, None) == 0, name          # c == 0


def test_ragged_entries_check_their_arguments_without_a_device(lib):
    buf = 0x1000
    for name in ("lshrs_cosine_ragged_i8", "lshrs_cosine_ragged_f8e4m3"):
        fn = getattr(lib, name)
        # (corpus, m, ldc, dim, queries, q, cand_rows, row_off, row_cnt, total, scores, err, stream)
        assert fn(None, 10, 8, 8, buf, 1, buf, buf, buf, 5, buf, buf, None) == BADARG, name
        assert fn(buf, 10, 4, 8, buf, 1, buf, buf, buf, 5, buf, buf, None) == BADARG, name
        assert fn(buf, 10, 8, 8, buf, 1, None, buf, buf, 5, buf, buf, None) == BADARG, name
        assert fn(buf, 10, 8, 8, buf, 1, buf, None, buf, 5, buf, buf, None) == BADARG, name
        assert fn(buf, 0, 8, 8, buf, 1, buf, buf, buf, 5, buf, buf, None) == BADARG, name
        assert fn(buf, 10, 16385, 16385, buf, 1, buf, buf, buf, 5, buf, buf, None) == TOOLARGE, name
        assert fn(None, 10, 8, 8, None, 0, None, None, None, 5, None, None, None) == 0, name
        assert fn(None, 10, 8, 8, None, 3, None, None, None, 0, None, None, None) == 0, name


def test_quantize_entries_check_their_arguments_without_a_device(lib):
    buf = 0x1000
    for name in QUANT:
        fn = getattr(lib, name)
        # (X, n, ldx, dim, out, ldo, status, stream)
        assert fn(None, 4, 8, 8, buf, 8, buf, None) == BADARG, name          # null input
        assert fn(buf, 4, 8, 8, None, 8, buf, None) == BADARG, name          # null output
        assert fn(buf, 4, 8, 8, buf, 8, None, None) == BADARG, name          # null status (required)
        assert fn(buf, 4, 7, 8, buf, 8, buf, None) == BADARG, name           # input stride < dim
        assert fn(buf, 4, 8, 8, buf, 7, buf, None) == BADARG, name           # output stride < dim
        assert fn(buf, 4, 8, 0, buf, 8, buf, None) == BADARG, name           # dim 0
        assert fn(buf, -1, 8, 8, buf, 8, buf, None) == BADARG, name          # negative rows
        assert fn(buf, 1 << 31, 8, 8, buf, 8, buf, None) == TOOLARGE, name   # one workgroup per row: < 2^31 rows
        assert fn(None, 0, 8, 8, None, 8, None, None) == 0, name             # no rows: nothing to do


def test_the_8bit_dtypes_sit_beside_the_16bit_ones():
    """similarity.corpus_entry reads both maps; the 16-bit one keeps its three entries (no GPU needed)."""
    from lshrs_amd import similarity

    assert similarity._CORPUS_ENTRY_8BIT == {"int8": "i8", "float8_e4m3fn": "f8e4m3"}
    assert similarity._CORPUS_ENTRY == {"float32": "f32", "bfloat16": "bf16", "float16": "f16"}
    import lshrs_amd

    assert lshrs_amd.quantize_rows is similarity.quantize_rows
