"""Putting a wide genome's per-group results back together: tensor plumbing, on any device.

The kernels place every chromosome on one 32-bit axis; a genome whose spans sum past 2^32 is answered chromosome
group by chromosome group (``HipEngine._wide`` over ``HipEngine._groups``).  Each function here takes the ``parts``
of such a run -- one ``(rows_a, rows_b, result)`` per group, in group order: the int64 ids that the group's rows have
in the whole tables, and what the operator returned for the sub-tables -- and returns what the operator returns for
the whole tables.  No group at all gives the operator's empty result.  Nothing here needs an engine or the library:
CPU tensors do (tests/test_wide_combine.py).
"""

from __future__ import annotations


def _cat(tensors, dtype, device):
    import torch

    return torch.cat(tensors) if tensors else torch.empty(0, dtype=dtype, device=device)


def pairs(parts, device):
    """INNER, CONTAINS and within-distance joins, result ``(local row_a, local row_b)``: the groups' pairs one after
    the other as int32 ids of the whole tables."""
    import torch

    return (_cat([ra[p[0].long()].to(torch.int32) for ra, _rb, p in parts], torch.int32, device),
            _cat([rb[p[1].long()].to(torch.int32) for _ra, rb, p in parts], torch.int32, device))


def per_row(parts, n: int, device):
    """COUNT and CLUSTER, result one int64 value per row of the group: the values in the order of the ``n`` rows of
    the whole table; a row of no group keeps 0."""
    import torch

    out = torch.zeros(n, dtype=torch.int64, device=device)
    for ra, _rb, values in parts:
        out[ra] = values
    return out


def nearest(parts, shape, device):
    """NEAREST, result ``(local idx_b, distance)`` of shape ``(n_a,)`` (k = 1) or ``(n_a, k)``: ``(idx_b int32,
    distance int64)`` of ``shape`` for the whole tables; a miss keeps idx_b -1 / distance 0."""
    import torch

    idx = torch.full(shape, -1, dtype=torch.int32, device=device)
    dist = torch.zeros(shape, dtype=torch.int64, device=device)
    for ra, rb, (gi, gd) in parts:
        hit = gi >= 0
        mapped = torch.full_like(gi, -1)
        if rb.numel():
            mapped[hit] = rb[gi[hit].long()].to(torch.int32)
        idx[ra] = mapped
        dist[ra] = gd
    return idx, dist


def row_ids(parts, device):
    """SEMI / ANTI, result local row ids of A: the whole table's, ascending, int32."""
    import torch

    return torch.sort(_cat([ra[rows.long()] for ra, _rb, rows in parts], torch.int64, device)).values.to(torch.int32)


def group_rows(parts, chrom, start, end):
    """GROUP BY interval, result ``(local group_of_row, local rep_row)``; ``chrom`` / ``start`` / ``end`` are the
    whole table's columns.  Each group numbers its groups along its own axis: they are renumbered in (chrom, start,
    end) order, which is the order of ``rep_row``."""
    import torch

    gid = torch.empty(chrom.shape[0], dtype=torch.int32, device=chrom.device)
    if not parts:
        return gid, gid.clone()
    rep = torch.cat([rows[r.long()] for rows, _rb, (_g, r) in parts])
    order = torch.argsort(end[rep], stable=True)
    order = order[torch.argsort(start[rep][order], stable=True)]
    order = order[torch.argsort(chrom[rep][order], stable=True)]
    rank = torch.empty_like(order)
    rank[order] = torch.arange(order.numel(), dtype=order.dtype, device=chrom.device)
    first = 0
    for rows, _rb, (g, r) in parts:
        gid[rows] = rank[first + g.long()].to(torch.int32)
        first += int(r.numel())
    return gid, rep[order].to(torch.int32)


def disjoin(parts, device):
    """DISJOIN, result ``(local parent, disjoin_start, disjoin_end)``: a group keeps (parent, start) order inside;
    the stable sort by parent restores it across the groups."""
    import torch

    parent = _cat([rt[p[0].long()] for rt, _rr, p in parts], torch.int64, device)
    order = torch.argsort(parent, stable=True)
    return (parent[order].to(torch.int32), _cat([p[1] for _rt, _rr, p in parts], torch.int32, device)[order],
            _cat([p[2] for _rt, _rr, p in parts], torch.int32, device)[order])


def _merge_columns(parts, device):
    """The groups' ``(chrom, start, end, count)`` one after the other, and the permutation that orders the regions by
    (chrom, start)."""
    import torch

    c, st, en = (_cat([p[k] for _rows, _rb, p in parts], torch.int32, device) for k in range(3))
    cnt = _cat([p[3] for _rows, _rb, p in parts], torch.int64, device)
    return (c, st, en, cnt), torch.argsort(c.long() * (1 << 32) + (st.long() + (1 << 31)), stable=True)


def merge(parts, device):
    """MERGE, result ``(chrom, start, end, count)`` of the group's regions: all regions ordered by (chrom, start)."""
    cols, order = _merge_columns(parts, device)
    return tuple(t[order] for t in cols)


#: the ``dtypes`` entry of :func:`merge_agg` for a STRING_AGG column
UTF8 = "utf8"


def utf8_in_order(columns, order, device):
    """Region-order concatenation of string results: ``columns`` holds one ``(offsets int32 [m_k + 1], data uint8)``
    per group, ``order`` indexes their rows laid end to end; returns ``(offsets, data)`` of the rows in that order,
    an Arrow utf8 layout with int32 offsets starting at 0.  The bytes move with one gather; a result past 2^31 - 1
    bytes does not fit one such column and is a ``ValueError``."""
    import torch

    lens = _cat([(o[1:] - o[:-1]).long() for o, _d in columns], torch.int64, device)
    first, base = [], 0   # where every row starts in the groups' bytes laid end to end
    for o, d in columns:
        first.append(o[:-1].long() + base)
        base += int(d.shape[0])
    first = _cat(first, torch.int64, device)
    data = _cat([d for _o, d in columns], torch.uint8, device)
    lens, first = lens[order], first[order]
    ends = torch.cumsum(lens, 0)
    total = int(ends[-1]) if ends.numel() else 0
    if total > 0x7FFFFFFF:
        raise ValueError(f"string aggregate of {total} bytes: exceeds one string column's 2^31 - 1 bytes")
    offsets = torch.zeros(lens.numel() + 1, dtype=torch.int32, device=device)
    offsets[1:] = ends.to(torch.int32)
    starts = ends - lens
    src = torch.repeat_interleave(first - starts, lens) + torch.arange(total, dtype=torch.int64, device=device)
    return offsets, data[src]


def merge_agg(parts, device, dtypes):
    """MERGE with aggregates, result ``(chrom, start, end, count, (values, valid), ...)``: a region never spans two
    groups, so the groups' regions are concatenated and every column takes :func:`merge`'s order.  ``dtypes``: the
    value dtype per aggregate (what no group at all returns); :data:`UTF8` marks a STRING_AGG column, whose result
    is ``(offsets, data, valid)`` and goes through :func:`utf8_in_order`."""
    import torch

    cols, order = _merge_columns(parts, device)
    aggs = []
    for j, dt in enumerate(dtypes):
        if dt == UTF8:
            valid = _cat([p[4 + j][2] for _rows, _rb, p in parts], torch.bool, device)[order]
            aggs.append(utf8_in_order([p[4 + j][:2] for _rows, _rb, p in parts], order, device) + (valid,))
        else:
            aggs.append((_cat([p[4 + j][0] for _rows, _rb, p in parts], dt, device)[order],
                         _cat([p[4 + j][1] for _rows, _rb, p in parts], torch.bool, device)[order]))
    return tuple(t[order] for t in cols) + tuple(aggs)
