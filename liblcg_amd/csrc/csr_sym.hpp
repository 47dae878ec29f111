// csr_sym.hpp -- the arithmetic of a symmetric run stretch (csr_sym.hip): which of a stretch's blocks read the half store, where a
// block's tile lies in it, which block a dispatched workgroup takes.  Plain C++ (host and device): tests/test_sym_map.py compiles
// it alone.  Not installed.
#pragma once

#if defined(__HIPCC__)
#define LCG_SYM_HD __host__ __device__
#else
#define LCG_SYM_HD
#endif

namespace lcgh {

// One symmetric run stretch as the product kernel sees it.  Blocks [inner0 - Q, inner0) are the APRON: they keep the old path and
// only lend their tiles to the partner reads of the blocks behind them.  Blocks [inner0, inner0 + NX * S) are the SLICED RANGE:
// NX slices of S consecutive blocks; dispatched workgroup w of the range works on block inner0 + (w % NX) * S + w / NX, so that
// workgroups w, w + NX, w + 2 NX ... (one XCD when NX = 8, two when NX = 4: workgroups are dealt round-robin over the eight) walk
// one slice front to back.  (One slice: the tiles are in block order and the workgroups are dealt by sym_group_block_of below.)
// Tile t of the half store holds one block's diagonal and p upper diagonals, diagonal-major: H[t][k][r], k = 0 .. p, r = 0 .. 63.
// The apron's tiles come first, in block order; block inner0 + e * S + j has tile Q + NX * j + e -- dispatch order, so the
// slices interleave in memory and the value stream stays one front in address space.
struct SymRun {
    int inner0 = 0;     // first block of the sliced range
    int S = 0;          // blocks per slice
    int NX = 0;         // slices: 1, 2, 4 or 8 (0: no symmetric stretch)
    int G = 1;          // one slice: consecutive blocks per XCD (sym_group_block_of), set where the product is launched
    int Q = 0;          // apron blocks = tiles in front of the sliced range's
    int p = 0;          // pairs of diagonals: L = 2 p + 1 entries per row, slot p the diagonal
    int TQ = 0;         // the offset of slot k lies at off[(k % 4) * TQ + k / 4] (the stretch's table: RunStretch::off, Q)
    const int *off = nullptr;
    const double *H = nullptr;
};

// off[0 .. L): a row's offsets column - row in storage order.  They must ASCEND strictly (CSR rows may be stored in any order, and a run
// block does not care: one that is not sorted is no symmetric stretch -- the apron below is sized from the last offset as the largest),
// with L = 2 p + 1, off[p] = 0 and off[2 p - k] = -off[k].
LCG_SYM_HD inline bool sym_offsets_ok(const int *off, int L)
{
    if (L < 1 || (L & 1) == 0) return false;
    const int p = L / 2;
    if (off[p] != 0) return false;
    for (int k = 1; k < L; k++)
        if (off[k] <= off[k - 1]) return false;
    for (int k = 0; k < p; k++)
        if (off[2 * p - k] != -off[k]) return false;
    return true;
}

// apron blocks for a largest offset of `maxoff` rows: every partner row of the block behind them lies in them
LCG_SYM_HD inline int sym_apron(int maxoff) { return (maxoff + 63) / 64 + 1; }

// The sliced range of the stretch [b0, b1): its first block (the first multiple of 8 with Q blocks of the stretch in front of it: the
// number of workgroups dispatched before it is a multiple of 8) and S.  false: fewer than NX blocks are left.
LCG_SYM_HD inline bool sym_range(int b0, int b1, int Q, int NX, int *inner0, int *S)
{
    const long first = ((long)b0 + Q + 7) / 8 * 8;
    if (NX < 1 || first + NX > (long)b1) return false;
    *inner0 = (int)first;
    *S = (int)((b1 - first) / NX);
    return true;
}

// block of dispatched workgroup w of the sliced range
LCG_SYM_HD inline int sym_block_of(int w, int inner0, int S, int NX)
{
    const int lg = NX == 8 ? 3 : NX == 4 ? 2 : NX == 2 ? 1 : 0;        // (NX is 1, 2, 4 or 8: no division in the kernel)
    return inner0 + (w & (NX - 1)) * S + (w >> lg);
}

// One slice, G consecutive blocks per XCD (G is 1, 2, 4 or 8): block of dispatched workgroup w.  Workgroups are dealt round-robin
// over the eight XCDs, so within every full window of 8 G blocks workgroup r of the window (XCD r % 8) takes block (r % 8) * G + r / 8
// of it: an XCD's G consecutive blocks are dispatched eight workgroups apart, and the 128-byte lines that two neighbouring blocks
// both read -- where a partner run or an x gather straddles them -- are fetched into ONE L2, once.  The blocks behind the last full
// window keep their order.  A permutation of the range; the tiles stay where they are (block b: tile Q + b - inner0).
LCG_SYM_HD inline int sym_group_block_of(int w, int inner0, int S, int G)
{
    const int lg = G == 8 ? 3 : G == 4 ? 2 : G == 2 ? 1 : 0, win = 8 << lg;
    if (w >= (S & ~(win - 1))) return inner0 + w;
    const int r = w & (win - 1);
    return inner0 + (w - r) + ((r & 7) << lg) + (r >> 3);
}

// tile of block b (an apron block or one of the sliced range)
LCG_SYM_HD inline int sym_tile_of(int b, int inner0, int S, int NX, int Q)
{
    const int d = b - inner0;
    if (d < 0 || NX == 1) return Q + d;
    const int e = d / S;
    return Q + NX * (d - e * S) + e;
}

} // namespace lcgh
