"""The host arithmetic of bsc_map_reduce's dispatcher, restated in plain Python: which kernel of csrc/bsc_fused.hip a
request runs on, with which grid, in how many splits, and how many trips of its outer loop the busiest wave or thread
makes.  Written the way `grid()` restates pass_grid in tests/test_regression_multi_tile_gpu.py; the line numbers are
those of csrc/bsc_fused.hip.

  normalise   map_normalise, 984-1048: sort_axes (927-935) by the output's strides (kept axes) or by the strides of the
              operand with the widest span (reduced axes), then coalesce (902-920).  A dense [R, C] request whose
              operands are all dense or scalar becomes rank 1; a row-vector operand stops that.
  map_pure    1190-1199: map_flat (1052-1085), map_is_dense (1088-1097), map_periodic (1102-1120), map_rows2d
              (1123-1158), map_dense (1161-1166), map_small (1169-1178), map_strided (1181-1188), in that order.
  reduce      reduce_plan (1210-1272), short_rows / reduce_short_rows (1289-1313), reduce_dense_wave (1315-1323),
              reduce_finish (1326-1332), map_reduce (1334-1362).

`plan` takes the request as bsc_map_reduce gets it (extents and per-operand strides of the kept and the reduced axes in
the caller's order, in elements), the alignment of every pointer as its offset mod 16 bytes, and the context: cu_count
and the options fused_map_blocks_per_cu, fused_waves_per_cu, rows_wg and fused_map_flat.  It returns a dict:

  kernel         the __global__ function's name
  linear         whether its LINEAR instantiation runs (None where the kernel has none)
  grid           (x, y) blocks of 256 threads
  splits         ranges the reduce axis is cut into (1 for the maps)
  lanes_per_row  the narrow kernel's L (0 elsewhere)
  col_chunk, chunks   map_rows_f32_kernel's columns per blockIdx.y and their count (0, 1 elsewhere)
  steps          the largest number of trips any wave or thread makes in the kernel's outer loop
  pstep          the periodic map's (stride * U) mod period4 (None elsewhere)
  unroll         U of the dense wave kernel (None elsewhere)
  finish         None, or {wave_per_output, grid, unrolled, steps} of map_reduce_finish_kernel (861-889)
  keep, red      the coalesced extents
"""
F32, F64 = "f32", "f64"
INT64_MAX = (1 << 63) - 1


def ceil_div(a, b):
    return -(-a // b)


def sort_axes(shape, rows, key):
    """927-935: a stable insertion sort of the axes by decreasing |stride| of row `key`, in place."""
    for a in range(1, len(shape)):
        b = a
        while b > 0 and abs(rows[key][b - 1]) < abs(rows[key][b]):
            shape[b], shape[b - 1] = shape[b - 1], shape[b]
            for row in rows:
                row[b], row[b - 1] = row[b - 1], row[b]
            b -= 1


def coalesce(shape, rows):
    """902-920: extent-1 axes go; (outer, inner) merge when every row has outer == inner * extent(inner)."""
    out_shape, out_rows = [], [[] for _ in rows]
    for a in range(len(shape)):
        if shape[a] == 1:
            continue
        merge = bool(out_shape) and all(o[-1] == r[a] * shape[a] for o, r in zip(out_rows, rows))
        if merge:
            out_shape[-1] *= shape[a]
            for o, r in zip(out_rows, rows):
                o[-1] = r[a]
        else:
            out_shape.append(shape[a])
            for o, r in zip(out_rows, rows):
                o.append(r[a])
    return out_shape, out_rows


def normalise(keep_shape, red_shape, keep_strides, red_strides, out_strides):
    """984-1048 -> (keep extents, red extents, kept strides per operand, reduced strides per operand, output strides),
    or None when there is nothing to run (n_out == 0, line 1022)."""
    n_in = len(keep_strides)
    n_out = 1
    for s in keep_shape:
        n_out *= s
    if n_out == 0:
        return None
    keep, red = list(keep_shape), list(red_shape)
    krows = [list(r) for r in keep_strides] + [list(out_strides)]
    rrows = [list(r) for r in red_strides]
    sort_axes(keep, krows, n_in)                                             # 1023
    if len(red) > 1:                                                         # 1024-1032
        key, best = 0, -1
        for k in range(n_in):
            span = sum(abs(rrows[k][a]) * (red[a] - 1) for a in range(len(red)))
            if span > best:
                best, key = span, k
        sort_axes(red, rrows, key)
    keep, krows = coalesce(keep, krows)                                      # 1033
    red, rrows = coalesce(red, rrows)
    return keep, red, krows[:n_in], rrows, krows[n_in]


def _stride(rows, k, a):
    """MapArgs pads shapes with 1 and strides with 0 beyond the rank (1035-1043)."""
    return rows[k][a] if a < len(rows[k]) else 0


def _prod(v):
    p = 1
    for s in v:
        p *= s
    return p


def _unrolled_trips(length, stride):
    """The generic reduce kernels' two loops (456-471, 831-846) and the finish kernel's (871-878), for the wave or lane
    that starts at 0: `for (; r + 3 stride < len; r += 4 stride)` then `for (; r < len; r += stride)`
    -> (trips of the first, trips of the second)."""
    first = max(0, ceil_div(length - 3 * stride, 4 * stride))
    rest = length - first * 4 * stride
    return first, max(0, ceil_div(rest, stride))


def _result(**kw):
    out = dict(kernel=None, linear=None, grid=(1, 1), splits=1, lanes_per_row=0, col_chunk=0, chunks=1, steps=1,
               pstep=None, unroll=None, finish=None)
    out.update(kw)
    return out


def plan(keep_shape, red_shape, keep_strides, red_strides, out_strides, align=None, linear=True, dtype=F32, special=False,
         cheap_pow=True, cu=256, fused_map_blocks_per_cu=8, fused_waves_per_cu=16, rows_wg=64, fused_map_flat=1):
    """`align`: offsets mod 16 bytes of the operands' pointers, then of the output's (default: all 0).  `linear`:
    linear_ops (955-963) holds for the request's ops.  `special`: lgamma / digamma among them.  `cheap_pow`: every pow
    has the exponent -1, 2, 0.5 or 1 (small_ok, 947)."""
    n_in = len(keep_strides)
    align = list(align) if align is not None else [0] * (n_in + 1)
    assert len(align) == n_in + 1 and len(red_strides) == n_in
    norm = normalise(keep_shape, red_shape, keep_strides, red_strides, out_strides)
    if norm is None:
        return _result(kernel=None, grid=(0, 0), steps=0, keep=[], red=[])
    keep, red, ks, rs, outs = norm
    n_out, n_red = _prod(keep), _prod(red)
    ctx = dict(cu=cu, blocks=fused_map_blocks_per_cu, waves=fused_waves_per_cu, rows_wg=rows_wg, flat=fused_map_flat)
    req = dict(keep=keep, red=red, ks=ks, rs=rs, outs=outs, n_out=n_out, n_red=n_red, n_in=n_in, in_ok=[a == 0 for a in align[:n_in]],
               out_ok=align[n_in] == 0, plain=(not special and dtype == F32), linear=bool(linear), cheap_pow=cheap_pow)
    res = _map_pure(req, ctx) if len(red_shape) == 0 else _map_reduce(req, ctx)      # 1378: the CALLER's rank_red
    res["keep"], res["red"] = keep, red
    return res


# ---- pure maps (1050-1199) ----------------------------------------------------------------------------------------------

def _map_pure(q, c):
    keep, ks, outs, n_in, n_out = q["keep"], q["ks"], q["outs"], q["n_in"], q["n_out"]
    rank = len(keep)
    cap = c["cu"] * c["blocks"]                                              # map_grid_cap, 966
    shape1 = keep[1] if rank > 1 else 1
    out0, out1 = (outs + [0, 0])[:2]

    # map_flat, 1052-1085
    if (q["plain"] and n_in <= 4 and n_out >= 4096 and n_out % 4 == 0 and n_out // 4 < (1 << 31) and q["out_ok"] and c["flat"] and
            (out0 == 1 if rank == 1 else rank == 2 and out1 == 1 and out0 == shape1 and shape1 % 4 == 0)):
        C = shape1 if rank == 2 else n_out
        took = True
        for k in range(n_in):
            s0 = _stride(ks, k, 0) if rank == 2 else 0
            s1 = _stride(ks, k, rank - 1)
            if rank == 1:
                kind = 0 if s1 == 1 else 1 if s1 == 0 else -1
            else:
                kind = 0 if (s0, s1) == (C, 1) else 1 if (s0, s1) == (0, 0) else 2 if (s0, s1) == (0, 1) else \
                    3 if (s0, s1) == (1, 0) else -1
            if kind < 0 or (kind in (0, 2) and not q["in_ok"][k]):
                took = False
                break
        if took:
            return _result(kernel="map_flat_f32_kernel", linear=q["linear"], grid=(ceil_div(n_out // 4, 1024), 1), steps=1)

    # map_is_dense, 1088-1097
    dense = q["plain"] and rank <= 1 and n_out % 4 == 0 and q["out_ok"] and (rank == 0 or out0 == 1)
    if dense:
        for k in range(n_in):
            s = _stride(ks, k, 0) if rank else 0
            if s != 0 and (s != 1 or not q["in_ok"][k]):
                dense = False
                break

    def dense_launch(period4=None):                                          # 1116-1117, 1162-1163; the loop at 193
        n4 = n_out // 4
        blocks = min(ceil_div(n4, 256), cap)
        sweep = blocks * 256 * 2                                             # stride * U, U = 2
        return _result(kernel="map_dense_f32_kernel", grid=(blocks, 1), steps=ceil_div(n4, sweep),
                       pstep=None if period4 is None else sweep % period4)

    if not dense:
        # map_periodic, 1102-1120
        C = shape1
        if (q["plain"] and rank == 2 and out1 == 1 and out0 == C and C % 4 == 0 and C <= (1 << 20) and (C < 256 or n_in > 3) and
                q["out_ok"]):
            took = True
            for k in range(n_in):
                s0, s1 = _stride(ks, k, 0), _stride(ks, k, 1)
                if (s0, s1) == (0, 0):
                    continue
                if not q["in_ok"][k] or (s0, s1) not in ((0, 1), (C, 1)):
                    took = False
                    break
            if took:
                return dense_launch(period4=C // 4)
        # map_rows2d, 1123-1158
        R = keep[0] if rank else 1
        if (q["plain"] and rank == 2 and n_in <= 3 and C % 4 == 0 and C >= 64 and out1 == 1 and out0 % 4 == 0 and q["out_ok"]):
            took = True
            for k in range(n_in):
                sc = _stride(ks, k, 1)
                if sc != 0 and (sc != 1 or _stride(ks, k, 0) % 4 != 0 or not q["in_ok"][k]):
                    took = False
                    break
            if took:
                blocks = max(1, min(ceil_div(R, 8), cap))
                chunks = 1
                if blocks < cap:
                    chunks = max(1, min(ceil_div(cap, blocks), ceil_div(C, 1024), 65535))
                col_chunk = ceil_div(ceil_div(C, chunks), 256) * 256
                chunks = ceil_div(C, col_chunk)
                return _result(kernel="map_rows_f32_kernel", grid=(blocks, chunks), col_chunk=col_chunk, chunks=chunks,
                               steps=ceil_div(R, blocks * 4 * 2))             # 390: rb += n_waves * U
    if dense:
        return dense_launch()
    # map_small, 1169-1178 (small_ok, 938-952)
    spans_ok = True
    for row in ks + [outs]:
        lo = sum(min(0, (keep[a] - 1) * row[a]) for a in range(rank))
        hi = sum(max(0, (keep[a] - 1) * row[a]) for a in range(rank))
        spans_ok = spans_ok and lo > -(1 << 30) and hi < (1 << 30)
    if q["plain"] and rank <= 2 and n_out <= (1 << 20) and n_in <= 4 and spans_ok and q["cheap_pow"]:
        return _result(kernel="map_small_f32_kernel", grid=(ceil_div(n_out, 256), 1), steps=1)
    # map_strided, 1181-1188
    blocks = min(ceil_div(n_out, 256), c["cu"] * 8)
    return _result(kernel="map_strided_kernel", grid=(blocks, 1), steps=ceil_div(n_out, blocks * 256))


# ---- map + reduce (1201-1362) ---------------------------------------------------------------------------------------------

def _map_reduce(q, c):
    keep, red, ks, rs, outs = q["keep"], q["red"], q["ks"], q["rs"], q["outs"]
    n_in, n_out, n_red = q["n_in"], q["n_out"], q["n_red"]
    # reduce_plan, 1210-1272: the fastest axis of the biggest operand decides
    big, big_elems = 0, -1.0
    for k in range(n_in):
        elems = 1.0
        for a in range(len(keep)):
            if ks[k][a] != 0:
                elems *= float(keep[a])
        for a in range(len(red)):
            if rs[k][a] != 0:
                elems *= float(red[a])
        if elems > big_elems:
            big_elems, big = elems, k
    min_keep = min([abs(s) for s in ks[big] if s != 0] or [INT64_MAX])
    min_red = min([abs(s) for s in rs[big] if s != 0] or [INT64_MAX])
    lanes_over_outputs = min_keep < min_red and n_out >= 16
    out0 = outs[0] if outs else 0
    dense_lane = (q["plain"] and lanes_over_outputs and n_in <= 3 and len(keep) == 1 and len(red) == 1 and n_out % 4 == 0 and
                  out0 == 1)
    dense_wave = q["plain"] and not lanes_over_outputs and n_in <= 3 and len(red) == 1 and n_red % 4 == 0
    bmask = 0
    for k in range(n_in):
        if dense_lane:
            sk = ks[k][0]
            if sk == 0:
                bmask |= 1 << k
            elif sk != 1 or not q["in_ok"][k] or rs[k][0] % 4 != 0:
                dense_lane = False
        if dense_wave:
            sr = rs[k][0]
            if sr == 0:
                bmask |= 1 << k
            else:
                if sr != 1 or not q["in_ok"][k]:
                    dense_wave = False
                if any(s % 4 != 0 for s in ks[k]):
                    dense_wave = False
    if bmask == (1 << n_in) - 1:                                             # 1253: nothing streams
        dense_lane = dense_wave = False
    narrow = dense_lane and n_out <= 128
    L = n_out // 4 if narrow else 0
    outs_per_block = (256 if dense_lane else 64) if lanes_over_outputs else 4
    jobs = ceil_div(n_out, outs_per_block)
    splits = 1
    want_blocks = c["cu"] * c["waves"] // 4
    if jobs < want_blocks:
        splits = want_blocks // jobs if lanes_over_outputs else (want_blocks * 4) // n_out
        max_splits = n_red // (16 * (64 // L) * 4 if narrow else 64 if lanes_over_outputs else 4096)
        splits = min(max(min(splits, max_splits), 1), 16384)

    finish = None
    if splits > 1:                                                           # reduce_finish, 1326-1332; the kernel, 861-889
        wave_per_output = n_out < 4096
        if wave_per_output:
            unrolled, tail = _unrolled_trips(splits, 64)
            finish = dict(wave_per_output=True, grid=ceil_div(n_out, 4), unrolled=unrolled, steps=unrolled + tail)
        else:
            finish = dict(wave_per_output=False, grid=ceil_div(n_out, 256), unrolled=0, steps=splits)
    common = dict(splits=splits, finish=finish)

    # map_reduce, 1334-1362
    if lanes_over_outputs:
        blocks = jobs * splits
        if narrow:                                                           # the loop at 750: 16 R rows per step
            R = 64 // L
            return _result(kernel="map_reduce_lane_narrow_f32_kernel", grid=(blocks, 1), lanes_per_row=L,
                           steps=ceil_div(n_red, splits * 16 * R), **common)
        if dense_lane:                                                       # 668: a block takes 16 rows per step
            return _result(kernel="map_reduce_lane_dense_f32_kernel", linear=bool(c["flat"] and q["linear"]), grid=(blocks, 1),
                           steps=ceil_div(n_red, splits * 16), **common)
        first, tail = _unrolled_trips(ceil_div(n_red, splits), 4)            # 819-846: wave 0 of split 0
        return _result(kernel="map_reduce_lane_kernel", grid=(blocks, 1), steps=first + tail, **common)
    blocks = ceil_div(n_out * splits, 4)
    if dense_wave and splits == 1 and len(keep) == 1 and n_red <= 1024 and n_out >= 4096 and c["flat"]:      # short_rows, 1289-1291
        rblocks = ceil_div(n_out, 16)                                        # reduce_short_rows, 1292-1313
        cap = c["cu"] * c["rows_wg"]
        if cap > 0 and rblocks > cap:
            rblocks = cap
        return _result(kernel="map_reduce_rows_f32_kernel", linear=q["linear"], grid=(rblocks, 1),
                       steps=ceil_div(n_out, rblocks * 4 * 4), **common)      # 574: r0 += n_waves * U
    if dense_wave:                                                           # reduce_dense_wave, 1315-1323; the loop at 506
        U = 1 if n_red <= 256 * splits else 4
        return _result(kernel="map_reduce_wave_dense_f32_kernel", linear=bool(U == 4 and c["flat"] and q["linear"]),
                       grid=(blocks, 1), unroll=U, steps=ceil_div(n_red // 4, splits * 64 * U), **common)
    first, tail = _unrolled_trips(ceil_div(n_red, splits), 64)               # 451-471: lane 0 of split 0
    return _result(kernel="map_reduce_wave_kernel", grid=(blocks, 1), steps=first + tail, **common)
