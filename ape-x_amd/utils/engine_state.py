"""Full-state checkpoints of the GPU engines: every persistent tensor of an engine (the HBM
replay with its frame ring and priority tree, the actor shard, the learner) streamed into one
directory, and loaded back IN PLACE -- captured hipGraphs hold the tensors' addresses.

Layout: ``<path>/data.bin`` (raw little-endian bytes, one extent per tensor, in sorted name
order) and ``<path>/manifest.pt`` -- a plain dict of ints, strings and lists that loads with
``torch.load(weights_only=True)``: the format version, the geometry the engine was built
with, the host scalars, and per tensor its dtype, shape, the leading rows saved, offset, byte
count and digest.

* Live rows only: a tensor may be given as ``(tensor, rows)``; only ``tensor[:rows]`` is written
  (a barely filled 10M-slot replay does not write 71 GB).  The rows not saved are left as the
  loading engine holds them; :func:`check_covers` refuses, before anything is overwritten, an
  engine that has written rows the checkpoint does not cover, so those are constructor values.
* Streaming: two pinned staging buffers of ``chunk_bytes``; the device copy of chunk i + 1 runs
  while chunk i is written to (or read from) the file.  No host copy of a whole tensor exists.
* Atomic: written into ``<path>.tmp/``, ``data.bin`` fsynced, the manifest written last; then
  an existing complete ``<path>`` becomes ``<path>.prev`` (an older ``.prev`` is dropped; a torn
  ``<path>`` is removed instead, so a complete ``.prev`` survives) and ``.tmp`` becomes ``<path>``.  A kill at any point leaves a complete ``<path>`` or a complete
  ``<path>.prev``; the loader falls back to ``.prev`` with a warning.
* Strict: the tensor name set, every dtype and shape and every geometry field must match, else
  :class:`CheckpointError` names the offender (before anything is overwritten).
* Integrity: after the copies every tensor's digest is recomputed where the tensor lives (the
  ``state_digest`` kernel on the GPU, :func:`digest_host` on the CPU) and compared.

The digest (:func:`digest_host` is its definition and the kernel's oracle): the bytes are read
as little-endian 64-bit words, the tail zero-padded; word ``i`` becomes
``mix64(word + (i + 1) * SALT)`` (the splitmix64 finalizer, a bijection); the terms are summed
modulo 2^64 and ``mix64(nbytes ^ LEN_SALT)`` is added.  The sum commutes -- any reduction order
gives the same value -- and the index salt makes it sensitive to position.
"""
from __future__ import annotations

import os
import shutil
import time
import warnings

import numpy as np
import torch

FORMAT_VERSION = 1
DATA_FILE = "data.bin"
MANIFEST_FILE = "manifest.pt"

DIGEST_SALT = 0x9E3779B97F4A7C15
DIGEST_LEN_SALT = 0xD6E8FEB86659FD93
_M1 = 0xBF58476D1CE4E5B9
_M2 = 0x94D049BB133111EB
_MASK = (1 << 64) - 1
_BLOCK_WORDS = 1 << 20


class CheckpointError(RuntimeError):
    """A checkpoint that does not fit the engine it is loaded into, or whose bytes are damaged."""


# ---------------------------------------------------------------------------- digest
def _mix64_int(x: int) -> int:
    x &= _MASK
    x ^= x >> 30
    x = (x * _M1) & _MASK
    x ^= x >> 27
    x = (x * _M2) & _MASK
    x ^= x >> 31
    return x


def _mix64(x: np.ndarray) -> np.ndarray:
    """splitmix64 finalizer over a uint64 array (array arithmetic wraps modulo 2^64)."""
    x = x ^ (x >> np.uint64(30))
    x = x * np.uint64(_M1)
    x = x ^ (x >> np.uint64(27))
    x = x * np.uint64(_M2)
    return x ^ (x >> np.uint64(31))


def digest_host(data) -> int:
    """The 64-bit state digest of a bytes-like object or uint8 array (see the module docstring)."""
    a = np.frombuffer(data, dtype=np.uint8) if not isinstance(data, np.ndarray) else data
    if a.dtype != np.uint8 or a.ndim != 1 or not a.flags.c_contiguous:
        raise ValueError("digest_host takes contiguous bytes")
    n = int(a.size)
    total = 0
    for w0 in range(0, -(-n // 8), _BLOCK_WORDS):
        part = a[8 * w0:8 * (w0 + _BLOCK_WORDS)]
        nw = -(-part.size // 8)
        if part.size != 8 * nw:  # the zero-padded tail
            part = np.concatenate([part, np.zeros(8 * nw - part.size, dtype=np.uint8)])
        words = part.view("<u8").astype(np.uint64)
        index = np.arange(w0 + 1, w0 + nw + 1, dtype=np.uint64)
        total += int(_mix64(words + index * np.uint64(DIGEST_SALT)).sum(dtype=np.uint64))
    return (total + _mix64_int(n ^ DIGEST_LEN_SALT)) & _MASK


def _bytes_view(t: torch.Tensor) -> torch.Tensor:
    if not t.is_contiguous():
        raise ValueError("the state digest and the checkpoint stream take contiguous tensors")
    return t.reshape(-1).view(torch.uint8)


def digest_tensor(t: torch.Tensor) -> int:
    """The digest of a contiguous tensor's bytes, computed where the tensor lives: one pass of
    the ``state_digest`` kernel on the GPU, :func:`digest_host` on the CPU."""
    b = _bytes_view(t)
    if b.is_cuda:
        from .. import ops

        with torch.cuda.device(b.device):
            return int(ops.hip().state_digest(b.data_ptr(), b.numel(), torch.cuda.current_stream().cuda_stream))
    return digest_host(b.numpy())


# ---------------------------------------------------------------------------- helpers
def _split(entry):
    """``tensor`` or ``(tensor, rows)`` -> (tensor, rows saved)."""
    t, rows = entry if isinstance(entry, tuple) else (entry, None)
    if t.dim() == 0:
        raise ValueError("state tensors have at least one dimension")
    full = int(t.shape[0])
    rows = full if rows is None else max(0, min(int(rows), full))
    return t, rows


def _staging(chunk_bytes: int, pinned: bool) -> list[torch.Tensor]:
    bufs = [torch.empty(chunk_bytes, dtype=torch.uint8) for _ in range(2)]
    return [b.pin_memory() for b in bufs] if pinned else bufs


def _pieces(extents, chunk_bytes: int):
    """(name, byte view of one chunk) over every extent, in file order."""
    for name, view in extents:
        for off in range(0, view.numel(), chunk_bytes):
            yield name, view[off:off + chunk_bytes]


def _fsync_dir(path: str) -> None:
    try:
        fd = os.open(path, os.O_RDONLY)
    except OSError:
        return
    try:
        os.fsync(fd)
    except OSError:
        pass
    finally:
        os.close(fd)


def _has_manifest(path: str) -> bool:
    return os.path.isfile(os.path.join(path, MANIFEST_FILE))


def resolve(path: str) -> str:
    """The directory to load: ``path`` when it holds a manifest, else a complete ``path.prev``
    (with a warning: the last save was torn), else :class:`CheckpointError`."""
    path = os.fspath(path).rstrip("/")
    if _has_manifest(path):
        return path
    prev = path + ".prev"
    if _has_manifest(prev):
        warnings.warn(f"{path} holds no manifest (torn save?): loading {prev}")
        return prev
    raise CheckpointError(f"no checkpoint manifest in {path} or {prev}")


def read_manifest(path: str) -> dict:
    return torch.load(os.path.join(resolve(path), MANIFEST_FILE), map_location="cpu", weights_only=True)


def check_covers(path: str, live_rows: dict) -> dict:
    """Before a load: the checkpoint must cover every row the loading engine has written
    (``live_rows``: tensor name -> leading rows it holds), so that the rows the checkpoint does
    not cover still hold their constructor values afterwards.  Raises :class:`CheckpointError`
    naming the tensor; nothing has been overwritten then.  Returns the manifest."""
    manifest = read_manifest(path)
    for name, rows in live_rows.items():
        e = manifest["tensors"].get(name)
        if e is not None and int(rows) > int(e["rows"]):
            raise CheckpointError(f"tensor {name!r}: the engine has already written {int(rows)} rows, the checkpoint "
                                  f"covers {e['rows']}")
    return manifest


# ---------------------------------------------------------------------------- save
def save_engine_state(path: str, tensors: dict, host: dict, geometry: dict, chunk_bytes: int = 64 << 20) -> dict:
    """Write ``tensors`` (name -> tensor or (tensor, rows)), the ``host`` scalars and the
    ``geometry`` as the checkpoint ``path``; returns the manifest with a ``timing`` entry
    (seconds waiting for device copies, writing the file, computing digests).  The caller has
    synchronised whatever writes the tensors."""
    path = os.fspath(path).rstrip("/")
    chunk_bytes = int(chunk_bytes)
    if chunk_bytes <= 0:
        raise ValueError("chunk_bytes must be positive")
    tmp, prev = path + ".tmp", path + ".prev"
    if os.path.isdir(tmp):
        shutil.rmtree(tmp)
    os.makedirs(tmp)
    timing = {"copy": 0.0, "write": 0.0, "digest": 0.0}
    entries, extents, offset = {}, [], 0
    cuda = False
    t0 = time.perf_counter()
    for name in sorted(tensors):
        t, rows = _split(tensors[name])
        view = _bytes_view(t[:rows])
        cuda = cuda or view.is_cuda
        entries[name] = {"dtype": str(t.dtype), "shape": [int(x) for x in t.shape], "rows": rows, "offset": offset,
                         "nbytes": int(view.numel()), "digest": f"{digest_tensor(t[:rows]):016x}"}
        extents.append((name, view))
        offset += int(view.numel())
    timing["digest"] = time.perf_counter() - t0
    bufs = _staging(chunk_bytes, cuda)
    events = [torch.cuda.Event(), torch.cuda.Event()] if cuda else None
    with open(os.path.join(tmp, DATA_FILE), "wb") as f:
        def flush(b: int, n: int) -> None:
            t1 = time.perf_counter()
            if events is not None:
                events[b].synchronize()
            t2 = time.perf_counter()
            f.write(memoryview(bufs[b][:n].numpy()))
            timing["copy"] += t2 - t1
            timing["write"] += time.perf_counter() - t2

        pending = None
        for i, (_, piece) in enumerate(_pieces(extents, chunk_bytes)):
            b, n = i & 1, piece.numel()
            bufs[b][:n].copy_(piece, non_blocking=True)   # chunk i + 1 travels while chunk i is written
            if events is not None:
                events[b].record()
            if pending is not None:
                flush(*pending)
            pending = (b, n)
        if pending is not None:
            flush(*pending)
        t1 = time.perf_counter()
        f.flush()
        os.fsync(f.fileno())
        timing["write"] += time.perf_counter() - t1
    manifest = {"version": FORMAT_VERSION, "geometry": dict(geometry), "host": dict(host), "tensors": entries,
                "total_bytes": offset}
    mpath = os.path.join(tmp, MANIFEST_FILE)
    with open(mpath + ".part", "wb") as f:   # the manifest last: its presence means the data is whole
        torch.save(manifest, f)
        f.flush()
        os.fsync(f.fileno())
    os.replace(mpath + ".part", mpath)
    _fsync_dir(tmp)
    if os.path.isdir(path):
        if _has_manifest(path):   # only a complete checkpoint becomes the fallback
            if os.path.isdir(prev):
                shutil.rmtree(prev)
            os.rename(path, prev)
        else:                     # torn or damaged: a complete .prev stays the fallback
            shutil.rmtree(path)
    os.rename(tmp, path)
    _fsync_dir(os.path.dirname(os.path.abspath(path)))
    return {**manifest, "timing": timing}


# ---------------------------------------------------------------------------- load
def _check(manifest: dict, tensors: dict, geometry: dict, data_bytes: int) -> None:
    if manifest.get("version") != FORMAT_VERSION:
        raise CheckpointError(f"checkpoint format version {manifest.get('version')!r}, this build reads "
                              f"{FORMAT_VERSION}")
    saved_geo = manifest["geometry"]
    for k in sorted(set(saved_geo) | set(geometry)):
        if k not in saved_geo or k not in geometry or saved_geo[k] != geometry[k]:
            raise CheckpointError(f"geometry field {k!r}: checkpoint has {saved_geo.get(k, '<absent>')!r}, the engine "
                                  f"{geometry.get(k, '<absent>')!r}")
    saved = manifest["tensors"]
    for name in sorted(set(saved) | set(tensors)):
        if name not in tensors:
            raise CheckpointError(f"tensor {name!r} is in the checkpoint but not in the engine")
        if name not in saved:
            raise CheckpointError(f"tensor {name!r} is in the engine but not in the checkpoint")
        t, _ = _split(tensors[name])
        e = saved[name]
        if e["dtype"] != str(t.dtype):
            raise CheckpointError(f"tensor {name!r}: checkpoint dtype {e['dtype']}, engine {t.dtype}")
        if list(e["shape"]) != [int(x) for x in t.shape]:
            raise CheckpointError(f"tensor {name!r}: checkpoint shape {list(e['shape'])}, engine {list(t.shape)}")
        if e["nbytes"] != _bytes_view(t[:e["rows"]]).numel():
            raise CheckpointError(f"tensor {name!r}: {e['nbytes']} bytes for {e['rows']} rows do not fit the engine's")
        if e["offset"] + e["nbytes"] > data_bytes:
            raise CheckpointError(f"tensor {name!r}: {DATA_FILE} is truncated ({data_bytes} bytes, the tensor ends at "
                                  f"{e['offset'] + e['nbytes']})")


def load_engine_state(path: str, tensors: dict, geometry: dict, chunk_bytes: int = 64 << 20) -> dict:
    """Load the checkpoint ``path`` into ``tensors`` in place (``copy_``) and return its host
    scalars.  Names, dtypes, shapes and geometry are checked before anything is overwritten;
    the digests after the copies: a mismatch raises :class:`CheckpointError` naming the tensor,
    and the tensors' contents are then undefined."""
    src = resolve(path)
    manifest = torch.load(os.path.join(src, MANIFEST_FILE), map_location="cpu", weights_only=True)
    data = os.path.join(src, DATA_FILE)
    _check(manifest, tensors, geometry, os.path.getsize(data) if os.path.isfile(data) else 0)
    saved = manifest["tensors"]
    order = sorted(saved, key=lambda k: saved[k]["offset"])
    extents = [(name, _bytes_view(_split(tensors[name])[0][:saved[name]["rows"]])) for name in order]
    cuda = any(v.is_cuda for _, v in extents)
    chunk_bytes = int(chunk_bytes)
    if chunk_bytes <= 0:
        raise ValueError("chunk_bytes must be positive")
    bufs = _staging(chunk_bytes, cuda)
    events = [torch.cuda.Event(), torch.cuda.Event()] if cuda else None
    used = [False, False]
    with open(data, "rb") as f:
        pos = 0
        for name in order:  # extents are contiguous in file order; seek only where they are not
            if saved[name]["offset"] != pos:
                raise CheckpointError(f"tensor {name!r}: extent at {saved[name]['offset']}, expected {pos}")
            pos += saved[name]["nbytes"]
        for i, (name, piece) in enumerate(_pieces(extents, chunk_bytes)):
            b, n = i & 1, piece.numel()
            if events is not None and used[b]:
                events[b].synchronize()           # the copy that last read this buffer is done
            got = f.readinto(memoryview(bufs[b][:n].numpy()))   # read chunk i + 1 while chunk i travels
            if got != n:
                raise CheckpointError(f"tensor {name!r}: {DATA_FILE} is truncated")
            piece.copy_(bufs[b][:n], non_blocking=True)
            if events is not None:
                events[b].record()
                used[b] = True
    if cuda:
        torch.cuda.synchronize()
    for name, view in extents:
        got = f"{digest_tensor(view):016x}"
        if got != saved[name]["digest"]:
            raise CheckpointError(f"tensor {name!r}: digest {got} after loading, the manifest has "
                                  f"{saved[name]['digest']} ({DATA_FILE} is damaged)")
    return dict(manifest["host"])
