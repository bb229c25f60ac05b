"""The id -> row table's C ABI and the Python boundary of ``DeviceVectors`` / ``LSHRS(keep_vectors=...)`` - what can be
checked without a GPU: the exports, the argument checks (which come before anything touches a device), the spread of the
hash (``lshrs_idmap_home_slot`` is the function the kernels call) and the constructors."""

from __future__ import annotations

import ctypes

import numpy as np
import pytest

NEW = ("lshrs_idmap_bytes", "lshrs_idmap_home_slot", "lshrs_idmap_insert_i64", "lshrs_idmap_erase_i64",
       "lshrs_idmap_lookup_i64", "lshrs_idmap_lookup_ragged_i64", "lshrs_idmap_rehash")
BADARG = -10001


@pytest.fixture(scope="module")
def lib():
    from lshrs_amd import _native

    _native.build()
    return _native.load()


def test_the_idmap_entries_are_exported(lib):
    from lshrs_amd import _native

    for name in NEW:
        assert name in _native.EXPORTS and hasattr(lib, name), name
    assert "idmap" in _native.UNITS
    assert lib.lshrs_abi_version() == _native.ABI_VERSION == 7


def test_argument_checks_come_before_the_device(lib):
    """NULL pointers, a negative n, a `slots` that is not a power of two: LSHRS_E_BADARG - on a machine without a GPU, so
    nothing was launched."""
    buf = (ctypes.c_int64 * 80)()
    base = (ctypes.addressof(buf) + 15) // 16 * 16           # a 16-byte aligned host block standing in for every array
    ok = 8
    assert lib.lshrs_idmap_bytes(8) == 128 and lib.lshrs_idmap_bytes(1 << 21) == 16 << 21
    for bad in (0, -8, 6, 12, (1 << 21) + 1):
        assert lib.lshrs_idmap_bytes(bad) == BADARG
        assert lib.lshrs_idmap_home_slot(5, bad) == BADARG
        assert lib.lshrs_idmap_insert_i64(base, bad, base, 1, 0, base, None) == BADARG
        assert lib.lshrs_idmap_erase_i64(base, bad, base, 1, base, None) == BADARG
        assert lib.lshrs_idmap_lookup_i64(base, bad, base, 1, base, None, None) == BADARG
        assert lib.lshrs_idmap_lookup_ragged_i64(base, bad, base, base, base, 1, 1, base, None, None) == BADARG
        assert lib.lshrs_idmap_rehash(base, bad, base + 256, ok, base, None) == BADARG
        assert lib.lshrs_idmap_rehash(base, ok, base + 256, bad, base, None) == BADARG
    assert lib.lshrs_idmap_home_slot(-1, ok) == BADARG
    # NULL pointers
    assert lib.lshrs_idmap_insert_i64(None, ok, base, 1, 0, base, None) == BADARG
    assert lib.lshrs_idmap_insert_i64(base, ok, None, 1, 0, base, None) == BADARG
    assert lib.lshrs_idmap_insert_i64(base, ok, base, 1, 0, None, None) == BADARG
    assert lib.lshrs_idmap_erase_i64(None, ok, base, 1, base, None) == BADARG
    assert lib.lshrs_idmap_erase_i64(base, ok, None, 1, base, None) == BADARG
    assert lib.lshrs_idmap_erase_i64(base, ok, base, 1, None, None) == BADARG
    assert lib.lshrs_idmap_lookup_i64(None, ok, base, 1, base, None, None) == BADARG
    assert lib.lshrs_idmap_lookup_i64(base, ok, None, 1, base, None, None) == BADARG
    assert lib.lshrs_idmap_lookup_i64(base, ok, base, 1, None, None, None) == BADARG
    for hole in range(5):
        args = [base, base, base, base, base]
        args[hole] = None
        assert lib.lshrs_idmap_lookup_ragged_i64(args[0], ok, args[1], args[2], args[3], 1, 1, args[4], None, None) == BADARG
    assert lib.lshrs_idmap_rehash(None, ok, base, ok, base, None) == BADARG
    assert lib.lshrs_idmap_rehash(base, ok, None, ok, base, None) == BADARG
    assert lib.lshrs_idmap_rehash(base, ok, base + 256, ok, None, None) == BADARG
    assert lib.lshrs_idmap_rehash(base, ok, base, ok, base, None) == BADARG       # onto itself
    # a negative n / q / first row, a table that is not 16-byte aligned
    assert lib.lshrs_idmap_insert_i64(base, ok, base, -1, 0, base, None) == BADARG
    assert lib.lshrs_idmap_insert_i64(base, ok, base, 1, -1, base, None) == BADARG
    assert lib.lshrs_idmap_erase_i64(base, ok, base, -1, base, None) == BADARG
    assert lib.lshrs_idmap_lookup_i64(base, ok, base, -1, base, None, None) == BADARG
    assert lib.lshrs_idmap_lookup_ragged_i64(base, ok, base, base, base, -1, 1, base, None, None) == BADARG
    assert lib.lshrs_idmap_lookup_ragged_i64(base, ok, base, base, base, 1, -1, base, None, None) == BADARG
    assert lib.lshrs_idmap_insert_i64(base + 8, ok, base, 1, 0, base, None) == BADARG
    assert lib.lshrs_idmap_lookup_i64(base + 8, ok, base, 1, base, None, None) == BADARG
    # nothing to do is not an error (and launches nothing)
    assert lib.lshrs_idmap_insert_i64(base, ok, base, 0, 0, base, None) == 0
    assert lib.lshrs_idmap_erase_i64(base, ok, base, 0, base, None) == 0
    assert lib.lshrs_idmap_lookup_i64(base, ok, base, 0, base, None, None) == 0
    assert lib.lshrs_idmap_lookup_ragged_i64(base, ok, base, base, base, 0, 0, base, None, None) == 0


def _murmur_home(ids: np.ndarray, slots: int) -> np.ndarray:
    x = ids.astype(np.uint64)
    x ^= x >> np.uint64(33)
    x *= np.uint64(0xff51afd7ed558ccd)
    x ^= x >> np.uint64(33)
    x *= np.uint64(0xc4ceb9fe1a85ec53)
    x ^= x >> np.uint64(33)
    return (x & np.uint64(slots - 1)).astype(np.int64)


def _probe_lengths(home: np.ndarray, slots: int) -> np.ndarray:
    """Linear-probing insertion of keys with these home slots, in order; the number of slots each one looked at (= what a
    later lookup of it looks at).  Vectorised by rounds: whoever finds its slot free takes it (first comer wins a tie), the
    rest step on."""
    taken = np.zeros(slots, dtype=bool)
    probes = np.ones(home.shape[0], dtype=np.int64)
    todo = np.arange(home.shape[0])
    at = home.copy()
    while todo.size:
        free = ~taken[at]
        # among the keys standing at one free slot, the first takes it
        cand = np.flatnonzero(free)
        _, first = np.unique(at[cand], return_index=True)
        won = cand[first]
        taken[at[won]] = True
        keep = np.ones(todo.size, dtype=bool)
        keep[won] = False
        todo, at = todo[keep], (at[keep] + 1) & (slots - 1)
        probes[todo] += 1
    return probes


def test_the_hash_spreads(lib):
    """1 000 000 ids into 2^21 slots (load 0.477), six id patterns: mean probes of a hit <= 1.6, no probe longer than 64
    (linear probing with a hash that spreads: 0.5 (1 + 1 / (1 - a)) = 1.46)."""
    n, slots = 1_000_000, 1 << 21
    rng = np.random.default_rng(7)
    base = np.arange(n, dtype=np.int64)
    rand40 = np.unique(rng.integers(0, 1 << 40, size=n + n // 8, dtype=np.int64))
    rng.shuffle(rand40)
    patterns = {
        "arange": base, "shift20": base << 20, "times_slots": base * slots, "times_3000017": base * 3_000_017,
        "high58": (1 << 58) + 4096 * base, "random40": rand40[:n],
    }
    assert patterns["random40"].shape[0] == n
    home_fn = np.vectorize(lambda i: lib.lshrs_idmap_home_slot(int(i), slots), otypes=[np.int64])
    for name, ids in patterns.items():
        home = home_fn(ids)                  # every home slot from the library: the function the kernels call
        assert np.array_equal(home, _murmur_home(ids, slots)), name      # (murmur3's 64-bit finalizer, low bits)
        probes = _probe_lengths(home, slots)
        print(f"{name}: mean probes {probes.mean():.4f}, longest {probes.max()}")
        assert probes.mean() <= 1.6, (name, probes.mean())
        assert probes.max() <= 64, (name, probes.max())


def test_device_vectors_argument_checks_need_no_gpu():
    from lshrs_amd import DeviceVectors

    for name in ("float32", "bfloat16", "float16", "int8", "float8_e4m3fn"):
        v = DeviceVectors(16, name)
        assert v.dtype == name and v.dim == 16 and len(v) == 0 and 5 not in v
        assert v.stats() == {"live": 0, "rows": 0, "dead": 0, "capacity": 0, "slots": 0, "bytes": 0}
    for bad in ("float64", "uint8", "float8_e5m2", "int4", ""):
        with pytest.raises(ValueError, match="dtype"):
            DeviceVectors(16, bad)
    with pytest.raises(ValueError):
        DeviceVectors(0)
    with pytest.raises(ValueError):
        DeviceVectors(16, capacity=-1)
    v = DeviceVectors(16, "bfloat16", capacity=100)
    x = np.ones((3, 16), dtype=np.float32)
    with pytest.raises(ValueError, match="shape"):
        v.add([1, 2, 3], np.ones((3, 15), dtype=np.float32))
    with pytest.raises(ValueError, match="shape"):
        v.add([1, 2, 3], np.ones(16, dtype=np.float32))
    with pytest.raises(ValueError, match="does not match"):
        v.add([1, 2], x)
    with pytest.raises(ValueError, match="non-negative"):
        v.add([1, -2, 3], x)
    assert len(v) == 0
    v.clear()
    assert v.remove([1, 2]) == 0


def test_add_without_a_gpu_raises(monkeypatch):
    import torch

    from lshrs_amd import DeviceVectors, NativeLibraryError, _native

    monkeypatch.setattr(_native, "_torch_ok", None)            # (whatever this machine has: no device is visible here)
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    v = DeviceVectors(16, "int8")
    with pytest.raises(NativeLibraryError):
        v.add([1, 2, 3], np.ones((3, 16), dtype=np.float32))
    with pytest.raises(NativeLibraryError):
        v.reserve(10)
    assert len(v) == 0


def test_keep_vectors_argument_checks_need_no_gpu(tmp_path):
    import pickle

    from lshrs_amd import LSHRS, DeviceVectors, InMemoryStorage

    plain = LSHRS(dim=32, num_perm=16, storage=InMemoryStorage())
    assert plain.vectors is None
    idx = LSHRS(dim=32, num_perm=16, storage=InMemoryStorage(), keep_vectors="bfloat16")
    assert isinstance(idx.vectors, DeviceVectors) and idx.vectors.dtype == "bfloat16" and idx.vectors.dim == 32
    own = DeviceVectors(32, "int8")
    assert LSHRS(dim=32, num_perm=16, storage=InMemoryStorage(), keep_vectors=own).vectors is own
    with pytest.raises(ValueError, match="dtype"):
        LSHRS(dim=32, num_perm=16, storage=InMemoryStorage(), keep_vectors="float64")
    with pytest.raises(ValueError, match="dimension"):
        LSHRS(dim=32, num_perm=16, storage=InMemoryStorage(), keep_vectors=DeviceVectors(31))
    with pytest.raises(ValueError, match="keep_vectors"):
        LSHRS(dim=32, num_perm=16, storage=InMemoryStorage(), keep_vectors=8)
    with pytest.raises(ValueError, match="dimension"):
        plain.set_corpus(DeviceVectors(31))
    plain.set_corpus(DeviceVectors(32))
    plain.set_corpus(None)
    # the store's kind travels with pickle and save_to_disk; the vectors do not
    back = pickle.loads(pickle.dumps(idx))
    assert back.vectors is not None and back.vectors.dtype == "bfloat16" and len(back.vectors) == 0
    assert pickle.loads(pickle.dumps(plain)).vectors is None
    idx.save_to_disk(tmp_path / "kept")
    loaded = LSHRS.load_from_disk(tmp_path / "kept", storage=InMemoryStorage())
    assert loaded.vectors is not None and loaded.vectors.dtype == "bfloat16"
    plain.save_to_disk(tmp_path / "plain")
    assert LSHRS.load_from_disk(tmp_path / "plain", storage=InMemoryStorage()).vectors is None
