"""A Python statement of which workgroup of the persistent fp16x3 linear (csrc/gemm_x3.hip, linear_f16x3_stream_kernel) computes which
256 x 256 output tile, and in which order - written from the launcher's arithmetic (linear_f16x3_impl: tiles_m, tiles_n, sup_n, sup_cols,
sup_rows, n_slots, grid) and the kernel's `decode` / `next_valid`, not by running either.  The GPU tests use it to PROVE that a shape
reaches a loop phase (a second tile, a middle tile, a half-wide tile that is not first), whatever the device's CU count.

    grid_for(cus, n_slots)          the launcher's grid: one workgroup per CU, a multiple of 8, at least 8, at most n_slots
    geometry(M, N)                  dict of tiles_m, tiles_n, sup_n, sup_cols, sup_rows, sup_m, n_slots
    decode(slot, geo)               (tm, tn) of a slot, or None where the slot holds no tile
    plan(M, N, grid)                per workgroup, the ordered list of valid (tm, tn) tiles (grid = the launch's gridDim.x)
    plan_for_cus(M, N, cus)         plan() with the grid the launcher picks on a device with `cus` compute units
    find_m(N, cus, want, m_max)     smallest ragged M (M % 256 == 1 + ...) whose plan satisfies the predicate `want(plan, geo)`
"""

BM = BN = 256            # G2_BM, G2_BN


def geometry(M, N):
    assert M >= 1 and N >= 128 and N % 128 == 0
    tiles_m, tiles_n = (M + BM - 1) // BM, (N + BN - 1) // BN
    sup_n = (tiles_n + 7) // 8
    sup_cols = (tiles_n + sup_n - 1) // sup_n
    sup_rows = 64 // sup_cols
    sup_m = (tiles_m + sup_rows - 1) // sup_rows
    n_slots = ((sup_m * sup_n + 7) // 8) * 8 * 64
    return dict(M=M, N=N, tiles_m=tiles_m, tiles_n=tiles_n, sup_n=sup_n, sup_cols=sup_cols, sup_rows=sup_rows, sup_m=sup_m, n_slots=n_slots)


def grid_for(cus, n_slots):
    grid = cus - cus % 8
    if grid < 8:
        grid = 8
    return min(grid, n_slots)


def decode(slot, geo):
    xcd, pos = slot & 7, slot >> 3
    sup, within = (pos >> 6) * 8 + xcd, pos & 63
    wr, wc = within // geo["sup_cols"], within % geo["sup_cols"]
    tm, tn = (sup // geo["sup_n"]) * geo["sup_rows"] + wr, (sup % geo["sup_n"]) * geo["sup_cols"] + wc
    if wr < geo["sup_rows"] and tm < geo["tiles_m"] and tn < geo["tiles_n"]:
        return tm, tn
    return None


def plan(M, N, grid):
    geo = geometry(M, N)
    assert grid >= 8 and grid % 8 == 0 and grid <= geo["n_slots"], (grid, geo["n_slots"])
    streams = []
    for wg in range(grid):
        tiles = []
        for slot in range(wg, geo["n_slots"], grid):
            t = decode(slot, geo)
            if t is not None:
                tiles.append(t)
        streams.append(tiles)
    return streams


def plan_for_cus(M, N, cus):
    return plan(M, N, grid_for(cus, geometry(M, N)["n_slots"]))


def is_half_wide(tile, geo):
    """The last column tile of an N that is an odd multiple of 128."""
    return geo["N"] % BN != 0 and tile[1] == geo["tiles_n"] - 1


def is_ragged_m(tile, geo):
    return geo["M"] % BM != 0 and tile[0] == geo["tiles_m"] - 1


def find_m(N, cus, want, m_max=40000, rem=1):
    """Smallest M = 256 (tiles_m - 1) + rem, searched over tiles_m, whose plan on a `cus`-CU device satisfies want(streams, geo)."""
    for tiles_m in range(1, (m_max + BM - 1) // BM + 1):
        M = BM * (tiles_m - 1) + rem
        if M > m_max:
            break
        geo = geometry(M, N)
        if want(plan(M, N, grid_for(cus, geo["n_slots"])), geo):
            return M
    return None
