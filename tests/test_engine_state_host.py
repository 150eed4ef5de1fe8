"""Host checks of ``utils/engine_state.py``: the digest's definition, the checkpoint format's
round trip on CPU tensors (live rows, chunk sizes that divide nothing), strict loading, damaged
and truncated data, torn saves and the ``.prev`` fallback."""
import os
import shutil
import warnings

import numpy as np
import pytest
import torch

from apex_amd.utils.engine_state import (DATA_FILE, MANIFEST_FILE, CheckpointError, check_covers, digest_host,
                                         digest_tensor, load_engine_state, save_engine_state)

GEO = {"capacity": 5, "frame_capacity": 5, "frame_bytes": 7056, "E": 2, "A": 3, "n_step": 3, "batch": 4,
       "params": 11, "staged": 0}


# ---------------------------------------------------------------------------- digest
def test_digest_mixes_the_length():
    assert digest_host(b"") != digest_host(b"\0")
    assert 0 <= digest_host(b"") < 1 << 64


def test_digest_zero_padded_tail_differs_from_explicit_zeros():
    data = bytes(range(1, 10))  # 9 bytes: the second word is padded with 7 zeros
    for extra in (1, 7, 8):
        assert digest_host(data) != digest_host(data + b"\0" * extra)


def test_digest_is_position_sensitive():
    rng = np.random.default_rng(0)
    a = rng.integers(0, 256, 64, dtype=np.uint8)
    b = a.copy()
    b[8:16], b[40:48] = a[40:48], a[8:16]
    assert not np.array_equal(a, b)
    assert digest_host(a) != digest_host(b)


def test_digest_sees_every_byte():
    rng = np.random.default_rng(1)
    a = rng.integers(0, 256, 4097, dtype=np.uint8)
    ref = digest_host(a)
    for i in range(a.size):
        a[i] ^= 0x10
        assert digest_host(a) != ref, i
        a[i] ^= 0x10
    assert digest_host(a) == ref


def test_digest_blocks_agree_with_the_word_loop():
    """The vectorised definition against a word-by-word Python loop (the formula as written)."""
    rng = np.random.default_rng(2)
    a = rng.integers(0, 256, 203, dtype=np.uint8)
    mask = (1 << 64) - 1

    def mix(x):
        x ^= x >> 30
        x = (x * 0xBF58476D1CE4E5B9) & mask
        x ^= x >> 27
        x = (x * 0x94D049BB133111EB) & mask
        return x ^ (x >> 31)

    padded = a.tobytes() + b"\0" * (-a.size % 8)
    total = 0
    for i in range(len(padded) // 8):
        w = int.from_bytes(padded[8 * i:8 * i + 8], "little")
        total += mix((w + (i + 1) * 0x9E3779B97F4A7C15) & mask)
    total += mix(a.size ^ 0xD6E8FEB86659FD93)
    assert digest_host(a) == total & mask


def test_digest_tensor_rejects_non_contiguous():
    t = torch.arange(12, dtype=torch.int32).reshape(3, 4)
    assert digest_tensor(t) == digest_host(t.numpy().tobytes())
    with pytest.raises(ValueError):
        digest_tensor(t.t())


# ---------------------------------------------------------------------------- round trip
def _tensors(seed: int) -> dict:
    g = torch.Generator().manual_seed(seed)
    return {
        "frames": torch.randint(0, 256, (5, 7056), dtype=torch.uint8, generator=g),
        "bytes": torch.randint(0, 256, (4099,), dtype=torch.uint8, generator=g),
        "ids": torch.randint(-5, 1 << 20, (7, 4), dtype=torch.int32, generator=g),
        "count": torch.randint(0, 1 << 40, (3,), dtype=torch.int64, generator=g),
        "reward": torch.randn(9, generator=g),
        "node_sum": torch.randn(6, dtype=torch.float64, generator=g),
        "empty": torch.zeros(0, 4, dtype=torch.float32),
    }


def _like(tensors: dict, fill: int) -> dict:
    return {k: torch.full_like(v, fill) for k, v in tensors.items()}


@pytest.mark.parametrize("chunk", [1000, 64 << 20])
def test_round_trip(tmp_path, chunk):
    src = _tensors(0)
    path = str(tmp_path / "ckpt")
    rows = {"frames": 3, "ids": 4, "reward": 0}
    out = save_engine_state(path, {k: (v, rows[k]) if k in rows else v for k, v in src.items()},
                            {"learn_steps": 12, "half": 1}, GEO, chunk_bytes=chunk)
    assert set(out["timing"]) == {"copy", "write", "digest"}
    manifest = torch.load(os.path.join(path, MANIFEST_FILE), weights_only=True)
    assert manifest["version"] == 1 and manifest["geometry"] == GEO
    assert manifest["tensors"]["frames"]["rows"] == 3 and manifest["tensors"]["frames"]["nbytes"] == 3 * 7056
    assert manifest["tensors"]["empty"]["nbytes"] == 0
    assert os.path.getsize(os.path.join(path, DATA_FILE)) == manifest["total_bytes"] \
        == sum(e["nbytes"] for e in manifest["tensors"].values())
    dst = _like(src, 7)
    host = load_engine_state(path, dst, GEO, chunk_bytes=chunk)
    assert host == {"learn_steps": 12, "half": 1}
    for k, v in src.items():
        n = rows.get(k, v.shape[0])
        assert dst[k].dtype == v.dtype and dst[k].shape == v.shape
        assert torch.equal(dst[k][:n], v[:n]), k
        assert torch.equal(dst[k][n:], torch.full_like(v[n:], 7)), k   # rows not saved are left alone


# ---------------------------------------------------------------------------- strictness
def _saved(tmp_path, name="ckpt"):
    src = _tensors(3)
    path = str(tmp_path / name)
    save_engine_state(path, src, {"learn_steps": 1}, GEO, chunk_bytes=1000)
    return path, src


def test_missing_and_extra_tensors(tmp_path):
    path, src = _saved(tmp_path)
    dst = _like(src, 0)
    del dst["reward"]
    with pytest.raises(CheckpointError, match="'reward'"):
        load_engine_state(path, dst, GEO)
    dst = _like(src, 0)
    dst["surplus"] = torch.zeros(2)
    with pytest.raises(CheckpointError, match="'surplus'"):
        load_engine_state(path, dst, GEO)


def test_shape_and_dtype_mismatch(tmp_path):
    path, src = _saved(tmp_path)
    dst = _like(src, 0)
    dst["ids"] = torch.zeros(7, 5, dtype=torch.int32)
    with pytest.raises(CheckpointError, match="'ids'"):
        load_engine_state(path, dst, GEO)
    dst = _like(src, 0)
    dst["count"] = torch.zeros(3, dtype=torch.int32)
    with pytest.raises(CheckpointError, match="'count'"):
        load_engine_state(path, dst, GEO)
    assert all(bool((v == 0).all()) for v in dst.values())   # nothing was overwritten


@pytest.mark.parametrize("field", sorted(GEO))
def test_geometry_mismatch_names_the_field(tmp_path, field):
    path, src = _saved(tmp_path)
    with pytest.raises(CheckpointError, match=f"'{field}'"):
        load_engine_state(path, _like(src, 0), {**GEO, field: GEO[field] + 1})
    missing = {k: v for k, v in GEO.items() if k != field}
    with pytest.raises(CheckpointError, match=f"'{field}'"):
        load_engine_state(path, _like(src, 0), missing)


# ---------------------------------------------------------------------------- damage
def test_changed_byte_names_the_tensor(tmp_path):
    path, src = _saved(tmp_path)
    manifest = torch.load(os.path.join(path, MANIFEST_FILE), weights_only=True)
    e = manifest["tensors"]["ids"]
    with open(os.path.join(path, DATA_FILE), "r+b") as f:
        f.seek(e["offset"] + e["nbytes"] // 2)
        b = f.read(1)
        f.seek(-1, os.SEEK_CUR)
        f.write(bytes([b[0] ^ 1]))
    with pytest.raises(CheckpointError, match="'ids'"):
        load_engine_state(path, _like(src, 0), GEO, chunk_bytes=1000)


def test_truncated_data_names_the_tensor(tmp_path):
    path, src = _saved(tmp_path)
    manifest = torch.load(os.path.join(path, MANIFEST_FILE), weights_only=True)
    last = max(manifest["tensors"], key=lambda k: manifest["tensors"][k]["offset"] + manifest["tensors"][k]["nbytes"])
    with open(os.path.join(path, DATA_FILE), "r+b") as f:
        f.truncate(manifest["total_bytes"] - 1)
    with pytest.raises(CheckpointError, match=f"'{last}'"):
        load_engine_state(path, _like(src, 0), GEO)


# ---------------------------------------------------------------------------- torn saves
def test_second_save_keeps_the_first_as_prev(tmp_path):
    path, first = _saved(tmp_path)
    second = _tensors(4)
    save_engine_state(path, second, {"learn_steps": 2}, GEO)
    assert not os.path.exists(path + ".tmp")
    dst = _like(first, 0)
    assert load_engine_state(path, dst, GEO) == {"learn_steps": 2}
    assert torch.equal(dst["ids"], second["ids"])
    assert load_engine_state(path + ".prev", dst, GEO) == {"learn_steps": 1}
    assert torch.equal(dst["ids"], first["ids"])
    save_engine_state(path, first, {"learn_steps": 3}, GEO)   # the older .prev is dropped
    assert load_engine_state(path + ".prev", dst, GEO) == {"learn_steps": 2}


def test_tmp_without_manifest_is_ignored(tmp_path):
    path, src = _saved(tmp_path)
    os.makedirs(path + ".tmp")
    with open(os.path.join(path + ".tmp", DATA_FILE), "wb") as f:
        f.write(b"half a save")
    dst = _like(src, 0)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        assert load_engine_state(path, dst, GEO) == {"learn_steps": 1}
    assert torch.equal(dst["frames"], src["frames"])
    save_engine_state(path, src, {"learn_steps": 5}, GEO)   # a stale .tmp does not stop the next save
    assert load_engine_state(path, dst, GEO) == {"learn_steps": 5}


def test_path_without_manifest_falls_back_to_prev(tmp_path):
    path, src = _saved(tmp_path)
    shutil.move(path, path + ".prev")
    os.makedirs(path)
    with open(os.path.join(path, DATA_FILE), "wb") as f:
        f.write(b"torn")
    dst = _like(src, 0)
    with pytest.warns(UserWarning, match="prev"):
        assert load_engine_state(path, dst, GEO) == {"learn_steps": 1}
    assert torch.equal(dst["node_sum"], src["node_sum"])
    shutil.rmtree(path + ".prev")
    with pytest.raises(CheckpointError):
        load_engine_state(path, dst, GEO)


def test_save_over_a_torn_path_keeps_the_complete_prev(tmp_path):
    path, first = _saved(tmp_path)
    shutil.move(path, path + ".prev")
    os.makedirs(path)
    with open(os.path.join(path, DATA_FILE), "wb") as f:
        f.write(b"torn")
    second = _tensors(4)
    save_engine_state(path, second, {"learn_steps": 2}, GEO)
    dst = _like(first, 0)
    assert load_engine_state(path, dst, GEO) == {"learn_steps": 2}
    assert load_engine_state(path + ".prev", dst, GEO) == {"learn_steps": 1}   # not replaced by the torn directory
    assert torch.equal(dst["ids"], first["ids"])


def test_check_covers_refuses_before_anything_is_overwritten(tmp_path):
    src = _tensors(0)
    path = str(tmp_path / "ckpt")
    save_engine_state(path, {k: (v, 3) if k == "frames" else v for k, v in src.items()}, {}, GEO)
    assert check_covers(path, {"frames": 3, "ids": 7})["tensors"]["frames"]["rows"] == 3
    with pytest.raises(CheckpointError, match="'frames'"):
        check_covers(path, {"frames": 4})
