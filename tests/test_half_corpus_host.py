"""The C ABI of the rerank on a 16-bit corpus (lshrs_cosine_{batch,ragged}_{bf16,f16}): declared in include/lshrs_hip.h,
bound in lshrs_amd/_native.py, exported by the library, and checking its arguments before anything touches a device.
CPU only - no kernel is launched here."""

from __future__ import annotations

import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "lshrs_hip.h")
NEW = ("lshrs_cosine_batch_bf16", "lshrs_cosine_batch_f16", "lshrs_cosine_ragged_bf16", "lshrs_cosine_ragged_f16")
BADARG, TOOLARGE = -10001, -10002


@pytest.fixture(scope="module")
def lib():
    from lshrs_amd import _native

    _native.build()
    return _native.load()


def test_the_four_entries_are_declared_bound_and_exported(lib):
    from lshrs_amd import _native

    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    out = subprocess.run(["nm", "-D", "--defined-only", _native.LIBRARY], capture_output=True, text=True, check=True)
    exported = {line.split()[-1] for line in out.stdout.splitlines() if " T " in line}
    for name in NEW:
        assert re.search(r"\bint\s+" + name + r"\s*\(\s*const uint16_t\* corpus,", text), name
        assert name in _native.EXPORTS and name in exported, name
        f32 = name.rsplit("_", 1)[0] + "_f32"
        assert getattr(lib, name).argtypes == getattr(lib, f32).argtypes, name      # the f32 entry's signature
    assert lib.lshrs_abi_version() == 7                                             # additive: the ABI number stays


def test_batch_entries_check_their_arguments_without_a_device(lib):
    buf = 0x1000                   # (never dereferenced: every call below returns before a launch)
    for name in ("lshrs_cosine_batch_bf16", "lshrs_cosine_batch_f16"):
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
    for name in ("lshrs_cosine_ragged_bf16", "lshrs_cosine_ragged_f16"):
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


def test_one_helper_decides_the_corpus_dtypes():
    """similarity.corpus_entry is where every caller learns which C entry reads a corpus (no GPU needed to refuse one)."""
    from lshrs_amd import similarity

    assert similarity._CORPUS_ENTRY == {"float32": "f32", "bfloat16": "bf16", "float16": "f16"}
    assert issubclass(similarity.CorpusError, TypeError) and issubclass(similarity.CorpusError, ValueError)
