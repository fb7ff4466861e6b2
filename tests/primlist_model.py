"""build_primary_list (csrc/pt_primlist.h) in NumPy: the per-pixel lists of grid spheres a pixel's primary rays can meet, as the
many-sphere kernel's workgroups build them.  The cones are float32, one ufunc per IEEE operation in the code's order
(rho, u, the wave's axis from its first and last `ok` lane, wr as the maximum over the wave); prim_cone_excludes is float64 on
the float32 operands, as in the code.  Waves are 64 consecutive lanes of workgroups of `threads` lanes, lane L of the launch
being tile pixel L; survivors of the wave's cone are collected in index order and the analysis gives up beyond 256; the lane's
list is a shift register, most recent first, and both table entries are encoded as csrc/pt_grid.h describes them.  No
transcendental on either side: tests/test_primary_exclusion_gpu.py requires equality with the device, word for word.
radius_factor and miss_scale are kPrimRadiusFactor and kPrimMissScale (PT_PRIMLIST_MUTANT=1: 0.3, =2: 0.64)."""
import numpy as np

import footprint_model as fm

f32, f64 = np.float32, np.float64
MAX_SURVIVORS, MAX_LIST = 256, 5
# why a lane has no list (the arms of build_primary_list), in the order the code decides them
INACTIVE, CONE_NAN_OR_WIDE, NO_OK_LANE, WAVE_WIDE, SURVIVORS, LIST_LONG, VALID = range(7)


def cone_excludes(geom, eye, axis, rho, miss_scale=1.0):
    """prim_cone_excludes for spheres geom = (x, y, z, rr) float32 [S] against cones (axis [3][L] float32, rho [L] float32):
    (miss [L][S], behind [L][S]) -- the sphere is excluded when either holds"""
    ex, ey, ez = f32(eye[0]), f32(eye[1]), f32(eye[2])
    off = [(c0 - g).astype(f32).astype(f64)[None, :] for c0, g in ((ex, geom[0]), (ey, geom[1]), (ez, geom[2]))]
    ux, uy, uz = (np.asarray(a, dtype=f32).astype(f64).reshape(-1, 1) for a in axis)
    rho = np.asarray(rho, dtype=f32).astype(f64).reshape(-1, 1)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        o2 = off[0] * off[0] + off[1] * off[1] + off[2] * off[2]
        uu = ux * ux + uy * uy + uz * uz
        hu = ux * off[0] + uy * off[1] + uz * off[2]
        rr = geom[3].astype(f64)[None, :] * f64(miss_scale)
        lo, lu = np.sqrt(o2), np.sqrt(uu)
        p2 = o2 - hu * hu / uu
        q = np.sqrt(np.where(p2 > 0.0, p2, 0.0)) - rho * lo
        miss = (q > 0.0) & (q * q - rr > 4.76837158203125e-06 * o2)                     # (M): 1.25 * 2^-18
        behind = (o2 - rr >= 0.00390625 * o2) & (hu > rho * lo * lu * 1.000001)          # (B)
    return miss, behind


def encode(k, s, slot):
    """The two table entries of a list of k spheres s[0..4] (most recent first) in the lane's slots `slot`, `slot + 1`: the entry
    format of csrc/pt_grid.h -- word 0 = first | link << 16 | count << 30, word 1 = second | third << 16; more than three: two
    spheres and the link to the second entry, which holds the rest"""
    k, slot = k.astype(np.uint32), slot.astype(np.uint32)
    s = [x.astype(np.uint32) for x in s]
    short = k <= 3
    e0x = np.where(short, s[0] | (k << np.uint32(30)), s[0] | ((slot + np.uint32(1)) << np.uint32(16)) | np.uint32(2 << 30))
    e0y = np.where(short, s[1] | (s[2] << np.uint32(16)), s[1])
    e1x = np.where(short, np.uint32(0), s[2] | ((k - np.uint32(2)) << np.uint32(30)))
    e1y = np.where(short, np.uint32(0), s[3] | (s[4] << np.uint32(16)))
    return np.stack([e0x, e0y, e1x, e1y], axis=-1).astype(np.uint32)


def decode(words):
    """The spheres a lane's two entries {e0.x, e0.y, e1.x, e1.y} list, read as the pooled walk reads the table: follow the link"""
    e0x, e0y, e1x, e1y = (int(w) for w in words)
    k, link = e0x >> 30, (e0x >> 16) & 0x1FFF
    got = [e0x & 0xFFFF, e0y & 0xFFFF, e0y >> 16][:k]
    if link:
        got += [e1x & 0xFFFF, e1y & 0xFFFF, e1y >> 16][:e1x >> 30]
    return got


def build_primary_lists(spheres, eye, basis, width, height, row_begin, row_end, threads, r_small, r_big, prim_base,
                        radius_factor=1.05, miss_scale=1.0):
    """Returns a dict over the LANES of the launch (the tile rounded up to `threads`): "words" uint32 [lanes][6] = {ok, k_out,
    e0.x, e0.y, e1.x, e1.y}, "why" (the arm that decided each lane), "rho" float32, "members" bool [lanes][n] (the spheres a lane's own cone KEEPS: its list where
    the list is valid, and what would have been on it where it is only too long), "analysed" bool [lanes] (the lanes that got as
    far as their own cone: `why` is VALID or LIST_LONG), "drop_M" / "drop_B" (how often a wave's cone and then a lane's own dropped a sphere by rule (M); by rule (B) alone)."""
    n = len(spheres)
    px = (row_end - row_begin) * width
    lanes = max((px + threads - 1) // threads, 1) * threads
    L = np.arange(lanes, dtype=np.int64)
    active = L < px
    row, col = (row_begin + L // width).astype(f32), (L % width).astype(f32)
    fac = f32(radius_factor)
    radius = spheres["radius"].astype(f32)
    pos = spheres["pos"].astype(f32)
    geom = (pos[:, 0], pos[:, 1], pos[:, 2], (radius * radius).astype(f32))
    in_grid = (radius >= f32(r_small)) & (radius <= f32(r_big))
    with np.errstate(invalid="ignore", divide="ignore", over="ignore", under="ignore"):
        d5 = fm.five_dirs(basis, width, height, row, col)
        dc = d5[0]
        lc = np.sqrt(fm._dot(dc, dc)).astype(f32)
        dev = np.zeros(lanes, dtype=f32)
        for k in range(4):
            e = [(d5[1 + k][i] - dc[i]).astype(f32) for i in range(3)]
            ln = np.sqrt(fm._dot(e, e)).astype(f32)
            dev = np.where(~(ln <= dev), ln, dev)
        rho = (((fac * dev).astype(f32) / lc).astype(f32) + f32(1e-6)).astype(f32)
        ok = active & (rho <= f32(0.125)) & (lc > 0) & (dev >= 0)
        inv = (f32(1.0) / lc).astype(f32)
        u = [(dc[i] * inv).astype(f32) for i in range(3)]
    why = np.where(active, np.where(ok, VALID, CONE_NAN_OR_WIDE), INACTIVE)
    k_lane = np.zeros(lanes, dtype=np.int64)
    s_regs = np.zeros((5, lanes), dtype=np.int64)
    members = np.zeros((lanes, n), dtype=bool)
    drops = {"M": 0, "B": 0}
    for w0 in range(0, lanes, 64):
        sl = slice(w0, w0 + 64)
        okw = ok[sl]
        idx = np.nonzero(okw)[0]
        if idx.size == 0:
            why[sl] = np.where(why[sl] == VALID, NO_OK_LANE, why[sl])
            continue
        l0, l1 = idx[0], idx[-1]
        with np.errstate(invalid="ignore", divide="ignore", over="ignore", under="ignore"):
            A = [f32(u[i][sl][l0] + u[i][sl][l1]) for i in range(3)]
            aa = f32(f32(f32(A[0] * A[0]) + f32(A[1] * A[1])) + f32(A[2] * A[2]))
            ia = f32(f32(1.0) / np.sqrt(aa).astype(f32))
            A = [f32(A[i] * ia) for i in range(3)]
            e = [(u[i][sl] - A[i]).astype(f32) for i in range(3)]
            wr_lane = np.where(okw, ((f32(1.05) * np.sqrt(fm._dot(e, e)).astype(f32)).astype(f32) + rho[sl]).astype(f32), f32(0.0))
            wr = np.fmax.reduce(wr_lane)                                      # fmaxf over the wave: NaN operands lose
        if not ((wr <= f32(0.25)) and (wr > f32(0.0))):
            why[sl] = np.where(okw, WAVE_WIDE, why[sl])
            continue
        miss, behind = cone_excludes(geom, eye, [np.full(1, A[i], dtype=f32) for i in range(3)], np.full(1, wr, dtype=f32), miss_scale)
        drops["M"] += int((in_grid & miss[0]).sum())
        drops["B"] += int((in_grid & behind[0] & ~miss[0]).sum())
        surv = np.nonzero(in_grid & ~(miss[0] | behind[0]))[0]               # index order (the ballot compaction keeps it)
        if surv.size > MAX_SURVIVORS:
            why[sl] = np.where(okw, SURVIVORS, why[sl])
            continue
        if surv.size == 0:
            continue
        g = tuple(x[surv] for x in geom)
        miss, behind = cone_excludes(g, eye, [dc[i][sl] for i in range(3)], rho[sl], miss_scale)
        keep = okw[:, None] & ~(miss | behind)                               # [64][S]
        drops["M"] += int((okw[:, None] & miss).sum())
        drops["B"] += int((okw[:, None] & behind & ~miss).sum())
        kk = keep.sum(axis=1)
        k_lane[sl] = kk
        from_end = np.cumsum(keep[:, ::-1], axis=1)[:, ::-1] * keep          # 1 = the most recently kept
        for m in range(5):
            hit = from_end == m + 1
            s_regs[m, sl] = np.where(hit.any(axis=1), surv[np.argmax(hit, axis=1)], 0)
        long_ = okw & (kk > MAX_LIST)
        why[sl] = np.where(long_, LIST_LONG, why[sl])
        members[w0 + np.nonzero(okw)[0][:, None], surv[None, :]] = keep[okw]
    ok_final = why == VALID
    kk = np.where(ok_final, k_lane, 0)
    slot = prim_base + 2 * (L % threads)
    words = np.empty((lanes, 6), dtype=np.uint32)
    words[:, 0] = ok_final
    words[:, 1] = kk
    words[:, 2:] = encode(kk, list(s_regs), slot)
    return {"words": words, "why": why, "rho": rho, "members": members, "drop_M": drops["M"], "drop_B": drops["B"], "lanes": lanes,
            "pixels": px, "analysed": (why == VALID) | (why == LIST_LONG)}
