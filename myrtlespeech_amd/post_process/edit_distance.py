"""Batched edit distance with operation counts on the device: ``ms_edit_distance`` (the specification is its comment in
include/ms_hotpath.h; tests/edit_distance_ref.py restates it).  The reference computes the same distances on the host, one
utterance at a time, with ``post_process/utils.py``'s ``levenshtein`` over lists of Python strings."""
from collections import namedtuple
from typing import Optional

import torch

from myrtlespeech_amd import _lib

MS_EDIT_TOKENS, MS_EDIT_WORDS = 0, 1
MAX_UNITS = 4096           # include/ms_hotpath.h MS_EDIT_MAX_LEN: units a side, by the row width
WAVE_UNITS = 63            # a side of at most this many units (by its row width) is served a wave per utterance

_INT_DTYPES = (torch.uint8, torch.int8, torch.int16, torch.int32, torch.int64)

# one row of ``edit_distance``'s result (or the sums of many): S + D + I == distance, hyp_units - I == ref_units - D
EditCounts = namedtuple("EditCounts", ["distance", "substitutions", "deletions", "insertions", "hyp_units", "ref_units"])

_workspace = _lib.Workspace()


def max_row_length(words: bool) -> int:
    """The widest row served: 4096 labels in token mode, 4096 one-letter words and their separators in word mode."""
    return 2 * MAX_UNITS - 1 if words else MAX_UNITS


def unit_capacity(width: int, words: bool) -> int:
    """Units a row of ``width`` labels can hold: what the kernel sizes its buffers and chooses its path by."""
    return (width + 1) // 2 if words else width


class _Side:
    """One operand after the host-side checks: ``mat`` [N, width] and ``lens`` [N], each on the host or on the device, and the
    host values of the lengths where they are known without a read-back."""

    def __init__(self, rows, lens, name: str, max_width: int):
        if isinstance(rows, (list, tuple)):
            rows = [r.tolist() if isinstance(r, torch.Tensor) else list(r) for r in rows]
            own = [len(r) for r in rows]
            width = max(own, default=0)
            mat = torch.zeros((len(rows), max(width, 1)), dtype=torch.int32)
            for n, r in enumerate(rows):
                if r:
                    mat[n, :len(r)] = torch.tensor(r, dtype=torch.int64).to(torch.int32)
            if lens is None:
                lens = torch.tensor(own, dtype=torch.int64)
            row_limit = torch.tensor(own, dtype=torch.int64)
        elif isinstance(rows, torch.Tensor):
            if rows.dtype not in _INT_DTYPES:
                raise ValueError(f"{name}.dtype={rows.dtype} must be an integer type")
            if rows.dim() != 2:
                raise ValueError(f"{name} must be [batch, max_length] (or a list of lists)")
            if lens is None:
                raise ValueError(f"{name}_lens is required with a tensor of rows")
            mat = rows.detach()
            row_limit = None
        else:
            raise ValueError(f"{name} must be a tensor or a list of lists, not {type(rows).__name__}")
        if not isinstance(lens, torch.Tensor):
            lens = torch.tensor(list(lens), dtype=torch.int64)
        if lens.dtype not in _INT_DTYPES:
            raise ValueError(f"{name}_lens.dtype={lens.dtype} must be an integer type")
        lens = lens.detach().reshape(-1)
        if lens.numel() != mat.shape[0]:
            raise ValueError(f"batch size of {name} ({mat.shape[0]}) and {name}_lens {lens.numel()} must be equal")
        host = _lib.cached_host(lens) if lens.is_cuda else lens
        if host is not None and host.numel():
            host = host.to(torch.int64).reshape(-1)
            if int(host.min()) < 0:
                raise ValueError(f"{name}_lens must not be negative")
            limit = row_limit if row_limit is not None else torch.full_like(host, mat.shape[1])
            if bool((host > limit).any()):
                raise ValueError(f"a value of {name}_lens exceeds the length of its row")
        self.mat, self.lens, self.host_lens, self.name = mat, lens, host, name
        # the width the kernel is given: rows wider than the limit are narrowed to the longest length where the host knows it
        self.width = mat.shape[1]
        if self.width > max_width and host is not None:
            self.width = max(int(host.max()) if host.numel() else 0, 1)
        if self.width > max_width:
            raise ValueError(f"{name}: rows of up to {max_width} labels are served, got {self.width}"
                             + ("" if host is not None else " columns with lengths known only to the device"))


def edit_distance(hyp, hyp_lens, ref, ref_lens, *, separator_index: Optional[int] = None, n_symbols: Optional[int] = None,
                  totals: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Edit distance and operation counts of every (hypothesis, reference) pair of a batch: ``[N, 6]`` int32 ON THE DEVICE,
    a row being an :class:`EditCounts`.  Nothing is read back and the host does not wait.

    ``hyp`` / ``ref``: integer label rows as a device tensor ``[N, width]`` (used as it is), a host tensor or a list of lists
    (padded; everything that starts on the host goes up in ONE staged copy); ``*_lens`` [N] (optional with lists).
    ``separator_index=None``: token mode, a unit is a label.  Otherwise word mode: labels outside ``[0, n_symbols)`` are dropped,
    the rest is cut into words at ``separator_index`` (-1: no separator), empty words are dropped.
    ``totals``: a device int64 ``[6]`` tensor to which the six column sums are added."""
    max_width = max_row_length(separator_index is not None)
    h, r = _Side(hyp, hyp_lens, "hyp", max_width), _Side(ref, ref_lens, "ref", max_width)
    if h.mat.shape[0] != r.mat.shape[0]:
        raise ValueError(f"batch size of hyp ({h.mat.shape[0]}) and ref ({r.mat.shape[0]}) must be equal")
    if separator_index is None:
        mode, separator, n_sym = MS_EDIT_TOKENS, -1, 0
    else:
        if n_symbols is None or int(n_symbols) < 0:
            raise ValueError("word mode (separator_index given) needs n_symbols >= 0")
        mode, separator, n_sym = MS_EDIT_WORDS, int(separator_index), int(n_symbols)
    if totals is not None and (not isinstance(totals, torch.Tensor) or totals.dtype != torch.int64 or totals.numel() != 6
                               or not totals.is_contiguous()):
        raise ValueError("totals must be a contiguous int64 tensor of 6 elements")
    _lib.require_gpu()
    if totals is not None and not totals.is_cuda:
        raise ValueError("totals must live on the device")
    batch = h.mat.shape[0]
    out = torch.empty((batch, 6), dtype=torch.int32, device="cuda")
    if batch == 0:
        return out
    # ONE staged upload for everything that starts on the host
    staged, where = [], {}
    for side in (h, r):
        for key, t in (("mat", side.mat[:, :side.width]), ("lens", side.lens)):
            if not t.is_cuda:
                where[(side.name, key)] = (sum(p.numel() for p in staged), t.shape)
                staged.append(t.to(torch.int32).reshape(-1))
    packed = _lib.upload(torch.cat(staged)) if staged else None

    def device(side, key, t):
        if (side.name, key) in where:
            start, shape = where[(side.name, key)]
            return packed[start:start + shape.numel()].reshape(shape)
        if key == "lens":
            return _lib.lens_i32(t)
        if t.shape[1] == 0:
            return torch.zeros((batch, 1), dtype=torch.int32, device="cuda")
        return t.to(torch.int32).contiguous()

    h_mat, h_len = device(h, "mat", h.mat[:, :h.width]), device(h, "lens", h.lens)
    r_mat, r_len = device(r, "mat", r.mat[:, :r.width]), device(r, "lens", r.lens)
    lib = _lib.load()
    ws = _workspace.get(lib.ms_edit_distance_workspace_bytes(batch, h_mat.shape[1], r_mat.shape[1]), zero=False)
    _lib.check(lib.ms_edit_distance(_lib.ptr(h_mat), h_mat.shape[1], _lib.ptr(h_len), _lib.ptr(r_mat), r_mat.shape[1],
                                    _lib.ptr(r_len), batch, mode, separator, n_sym, _lib.ptr(out), _lib.ptr(totals),
                                    _lib.ptr(ws), ws.numel(), _lib.stream_ptr()), "ms_edit_distance")
    return out
