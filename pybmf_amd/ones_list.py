"""The ones of a bit matrix as the row list the trace-form thresholding objectives walk (csrc/thresh_trace.hip, thresh_wide.hip,
thresh_cols.hip): column indices row after row, cut into segments of at most 128 cells of one row, the longest first."""
from __future__ import annotations

import torch

SEG = 128   # cells of a segment: a wave's unit of work


def list_fits(n_ones: int, free_bytes: int) -> bool:
    """The list costs ~16 bytes per one while it is built: it may take a quarter of the free device memory, at most 4 GiB."""
    return int(n_ones) * 16 <= min(int(free_bytes) // 4, 4 << 30)


def ones_segments(B, m: int, n: int):
    """(seg_row int32, seg_beg int64, seg_len int32, nseg, idx int32) of the ones of rows [0, m), columns [0, n) of BitMatrix B, on
    B.device (the caller has made it current)."""
    dev = B.device
    shifts = torch.arange(32, dtype=torch.int32, device=dev)
    step = max(1, (1 << 26) // max(1, B.bits.shape[1] * 32))   # rows per chunk: the unpacked 0 / 1 chunk stays under 256 MB
    rows_l, cols_l = [], []
    for a in range(0, m, step):
        b = min(m, a + step)
        cells = ((B.bits[a:b].unsqueeze(-1) >> shifts) & 1).reshape(b - a, -1)[:, :n]   # rows a..b of X as 0 / 1
        rc = torch.nonzero(cells)                                                       # row-major order
        rows_l.append(rc[:, 0] + a)
        cols_l.append(rc[:, 1].to(torch.int32))
        del cells, rc
    rows_all = torch.cat(rows_l) if rows_l else torch.zeros(0, dtype=torch.int64, device=dev)
    idx = (torch.cat(cols_l) if cols_l else torch.zeros(0, dtype=torch.int32, device=dev)).contiguous()
    counts = torch.bincount(rows_all, minlength=m)
    starts = torch.cumsum(counts, 0) - counts
    nseg_row = (counts + SEG - 1) // SEG
    seg_row = torch.repeat_interleave(torch.arange(m, device=dev), nseg_row)
    first = torch.cumsum(nseg_row, 0) - nseg_row
    within = torch.arange(seg_row.numel(), device=dev) - first[seg_row]
    seg_beg = starts[seg_row] + within * SEG
    seg_len = torch.minimum(counts[seg_row] - within * SEG, torch.tensor(SEG, device=dev))
    o = torch.argsort(seg_len, descending=True, stable=True)
    seg_row, seg_beg, seg_len = seg_row[o].to(torch.int32).contiguous(), seg_beg[o].contiguous(), seg_len[o].to(torch.int32).contiguous()
    return seg_row, seg_beg, seg_len, int(seg_row.numel()), idx
