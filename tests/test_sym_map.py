"""The arithmetic of a symmetric run stretch (liblcg_amd/csrc/csr_sym.hpp) compiled alone with g++ and compared with a restatement in
Python: the antisymmetry test of an offset table, the apron, the sliced range with its alignment to eight blocks, the block of a
dispatched workgroup and the tile of a block -- which must be dispatch order, and one tile per block."""
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SRC = r"""
#include <cstdio>
#include <cstdlib>
#include "csr_sym.hpp"
using namespace lcgh;
int main(int argc, char **argv)
{
    if (argv[1][0] == 'o') {            // o L off...
        const int L = atoi(argv[2]);
        int off[64];
        for (int k = 0; k < L; k++) off[k] = atoi(argv[3 + k]);
        printf("%d\n", sym_offsets_ok(off, L) ? 1 : 0);
        return 0;
    }
    const int b0 = atoi(argv[2]), b1 = atoi(argv[3]), maxoff = atoi(argv[4]), NX = atoi(argv[5]);
    const int Q = sym_apron(maxoff);
    int inner0 = -1, S = -1;
    if (!sym_range(b0, b1, Q, NX, &inner0, &S)) { printf("none %d\n", Q); return 0; }
    printf("%d %d %d\n", Q, inner0, S);
    for (int w = 0; w < NX * S; w++) printf("%d ", sym_block_of(w, inner0, S, NX));
    printf("\n");
    for (int b = inner0 - Q; b < inner0 + NX * S; b++) printf("%d ", sym_tile_of(b, inner0, S, NX, Q));
    printf("\n");
    return 0;
}
"""


def _exe(tmp_path_factory):
    d = tmp_path_factory.mktemp("sym_map")
    src = d / "sym_map.cpp"
    src.write_text(SRC)
    exe = d / "sym_map"
    subprocess.check_call(["g++", "-O1", "-std=c++11", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "liblcg_amd", "csrc"), str(src), "-o", str(exe)])
    return str(exe)


def plan(b0, b1, maxoff, nx):
    """The restatement: apron, first block of the sliced range, blocks per slice (None: fewer than nx blocks are left)."""
    Q = -(-maxoff // 64) + 1
    inner0 = -(-(b0 + Q) // 8) * 8
    if inner0 + nx > b1:
        return Q, None, None
    return Q, inner0, (b1 - inner0) // nx


def test_offsets(tmp_path_factory):
    exe = _exe(tmp_path_factory)
    cases = [([0], 1), ([-5, 0, 5], 1), ([-70, -3, 0, 3, 70], 1), ([-70, 0, 50], 0), ([-5, 0], 0), ([0, 5, 10], 0), ([-5, 1, 5], 0),
             ([-70, -3, 0, 4, 70], 0), ([5, 0, -5], 0),
             ([-1, -500, 0, 500, 1], 0), ([-3, -3, 0, 3, 3], 0), ([-500, -1, 0, 1, 500], 1)]      # (mirror order, not ascending: the apron would be sized from 1)
    for off, want in cases:
        out = subprocess.check_output([exe, "o", str(len(off))] + [str(o) for o in off], text=True)
        assert int(out) == want, (off, out)


def test_ranges_blocks_and_tiles(tmp_path_factory):
    exe = _exe(tmp_path_factory)
    for b0, b1, maxoff, nx in [(4, 60, 200, 8), (4, 60, 200, 1), (1, 23, 64, 8), (1, 23, 63, 8), (2, 17, 65, 8), (3, 16, 1, 8), (0, 9, 0, 1),
                               (3, 13, 1, 8), (5, 37, 130, 8), (6, 50, 129, 8), (2, 1000, 190, 8), (4, 61, 200, 2), (4, 61, 200, 4),
                               (1, 11, 64, 4), (1, 9, 64, 2), (1, 8, 64, 2)]:
        out = subprocess.check_output([exe, "r", str(b0), str(b1), str(maxoff), str(nx)], text=True).splitlines()
        Q, inner0, S = plan(b0, b1, maxoff, nx)
        if inner0 is None:
            assert out[0].split() == ["none", str(Q)], (b0, b1, maxoff, nx, out)
            continue
        assert [int(v) for v in out[0].split()] == [Q, inner0, S], (b0, b1, maxoff, nx, out[0])
        assert inner0 % 8 == 0 and inner0 - Q >= b0 and inner0 + nx * S <= b1 and b1 - (inner0 + nx * S) < nx
        # every partner row of the first sliced block lies in the apron
        assert 64 * inner0 - maxoff >= 64 * (inner0 - Q)
        blocks = np.array(out[1].split(), np.int64)
        w = np.arange(nx * S)
        assert np.array_equal(blocks, inner0 + (w % nx) * S + w // nx)
        assert np.array_equal(np.sort(blocks), np.arange(inner0, inner0 + nx * S))       # every block once
        tiles = np.array(out[2].split(), np.int64)
        assert np.array_equal(tiles[:Q], np.arange(Q))                                   # the apron first, in block order
        assert np.array_equal(tiles[Q:][blocks - inner0], Q + w)                         # then dispatch order: workgroup w's block has tile Q + w
        assert np.array_equal(np.sort(tiles), np.arange(Q + nx * S))                     # one tile per block
