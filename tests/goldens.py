"""Recorded results of the reference implementation (``tests/golden/*.npz``).

The differential host tests compare this framework with what the reference's own classes
computed for the same seeded inputs.  ``scripts/make_golden.py --reference DIR`` records
those results by driving the reference objects through the ``_drive_*`` / ``_ref_*``
functions of the test modules (the same drivers the tests run on this framework's
objects); the tests read only the recorded arrays, so the suite needs no copy of the
reference.  Only data is stored: inputs, weights and outputs, never reference code.
"""
from __future__ import annotations

import os

import numpy as np

DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def path(name: str) -> str:
    return os.path.join(DIR, name + ".npz")


def load(name: str) -> dict:
    with np.load(path(name), allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


def save(name: str, arrays: dict) -> str:
    os.makedirs(DIR, exist_ok=True)
    np.savez(path(name), **{k: np.asarray(v) for k, v in arrays.items()})
    return path(name)


def put_state(arrays: dict, prefix: str, state: dict) -> None:
    """A torch state_dict (or name -> tensor / None map) under ``prefix``; ``None`` entries
    (a parameter without gradient) are recorded by name in ``<prefix>__none``."""
    none = []
    for k, v in state.items():
        if v is None:
            none.append(k)
        else:
            arrays[f"{prefix}/{k}"] = v.detach().cpu().numpy().copy()  # (a snapshot: the model trains on)
    arrays[f"{prefix}__keys"] = np.array(list(state), dtype=np.str_)
    arrays[f"{prefix}__none"] = np.array(none, dtype=np.str_)


def get_state(arrays: dict, prefix: str) -> dict:
    """Inverse of ``put_state``: name -> torch tensor (or None), in the recorded key order."""
    import torch

    none = set(arrays[f"{prefix}__none"].tolist())
    return {str(k): (None if str(k) in none else torch.from_numpy(arrays[f"{prefix}/{k}"].copy()))
            for k in arrays[f"{prefix}__keys"].tolist()}
