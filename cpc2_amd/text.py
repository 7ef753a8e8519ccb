"""Decimal text of a device matrix (csrc/text.hip): the `fea` lines of cpc2_amd.eval.build_zeroSpeech_features.

    format_rows(x, prefix=None) -> uint8 device tensor
    write_rows(file, buf)          the buffer through pinned host memory into an open binary file

Row r of the text is prefix[r], a blank, the values of the row joined by blanks, and a newline; without prefixes a row starts
at its first value.  A float32 value is written as CPython writes repr(float(v)) -- byte for byte, whatever the value -- and
an int64 value as str(int(v)).  The reference builds these lines in the interpreter, one str() per value
(cpc/eval/build_zeroSpeech_features.py:70-77); here one thread does a value.  There is no CPU fallback.
"""
import time

import torch

from . import _lib

SLOT_BYTES = 24              # bytes a value's text may take (the longest are 23: -1.1754943508222875e-38)


def _prefix_tables(prefix, rows, device):
    """The prefixes as one byte vector and rows + 1 offsets into it, on the device."""
    if isinstance(prefix, (str, bytes)) or len(prefix) != rows:
        raise ValueError(f"format_rows: prefix must hold one string per row ({rows}), got "
                         f"{'one string' if isinstance(prefix, (str, bytes)) else len(prefix)}")
    parts = [p.encode() if isinstance(p, str) else bytes(p) for p in prefix]
    if any(b"\n" in p for p in parts):
        raise ValueError("format_rows: a prefix holds a newline")
    offsets = [0]
    for p in parts:
        offsets.append(offsets[-1] + len(p))
    data = torch.frombuffer(bytearray(b"".join(parts) + b"\0"), dtype=torch.uint8)         # (never empty: the kernel takes its address)
    return data.to(device), torch.tensor(offsets, dtype=torch.int64).to(device)


def format_rows(x, prefix=None):
    """x: [rows, cols] float32 or int64 on the device; prefix: None or one str / bytes per row.  Returns the text as a
    uint8 device tensor (empty for zero rows).  The same input gives the same bytes, call after call."""
    if not torch.is_tensor(x) or x.dtype not in (torch.float32, torch.int64):
        raise TypeError(f"format_rows takes a float32 or an int64 tensor, got {x.dtype if torch.is_tensor(x) else type(x).__name__}")
    _lib.require_gpu(x)
    if x.dim() != 2 or x.size(1) < 1:
        raise ValueError(f"format_rows takes a matrix [rows, cols >= 1], got {tuple(x.shape)}")
    rows, cols = x.shape
    device = x.device
    if prefix is not None:
        prefix_data, prefix_off = _prefix_tables(prefix, rows, device)
    if rows == 0:
        return torch.empty(0, dtype=torch.uint8, device=device)
    x = x.contiguous()
    lib, st = _lib.load(), _lib.stream_ptr(device)
    with torch.cuda.device(device):
        slots = torch.empty(rows * cols * (SLOT_BYTES // 8), dtype=torch.int64, device=device)
        lens = torch.empty(rows * cols, dtype=torch.uint8, device=device)
        entry = lib.cpc_text_format_f32 if x.dtype == torch.float32 else lib.cpc_text_format_i64
        _lib.check(entry(_lib.ptr(x), rows * cols, _lib.ptr(slots), _lib.ptr(lens), st), "text_format")
        row_bytes = torch.empty(rows, dtype=torch.int64, device=device)
        p_data, p_off = (_lib.ptr(prefix_data), _lib.ptr(prefix_off)) if prefix is not None else (_lib.ptr(None), _lib.ptr(None))
        _lib.check(lib.cpc_text_row_bytes(_lib.ptr(lens), rows, cols, p_off, _lib.ptr(row_bytes), st), "text_row_bytes")
        row_end = torch.cumsum(row_bytes, 0)
        row_off = row_end - row_bytes                                  # the exclusive scan
        total = int(row_end[-1])
        out = torch.empty(total, dtype=torch.uint8, device=device)
        _lib.check(lib.cpc_text_pack(_lib.ptr(slots), _lib.ptr(lens), rows, cols, p_data, p_off, _lib.ptr(row_off), _lib.ptr(out),
                                     total, st), "text_pack")
    return out


def write_rows(file, buf, timings=None):
    """Writes a device byte buffer to `file` (open for binary writing) through pinned host memory; returns the bytes written.
    timings: a dict whose "copy" and "write" entries receive the seconds of the two halves."""
    t0 = time.perf_counter()
    host = torch.empty(buf.numel(), dtype=torch.uint8, pin_memory=buf.is_cuda and buf.numel() > 0)
    host.copy_(buf)
    t1 = time.perf_counter()
    file.write(memoryview(host.numpy()))
    if timings is not None:
        timings["copy"] = timings.get("copy", 0.0) + t1 - t0
        timings["write"] = timings.get("write", 0.0) + time.perf_counter() - t1
    return buf.numel()
