"""Consecutive blocks per XCD in the symmetric product's one slice (liblcg_amd/csrc/csr_sym.hpp: sym_group_block_of), compiled alone
with g++ as test_sym_map.py does.  For every range length S = 1 .. 40 (and some longer ones) and G = 1, 2, 4, 8: the workgroups
take every block of the range exactly once; in every full window of 8 G blocks the workgroups of one XCD (w % 8: workgroups are
dealt round-robin) take G consecutive blocks, in ascending order, and the eight XCDs' runs tile the window; the blocks behind the
last full window, and all of them at G = 1, keep their order."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SRC = r"""
#include <cstdio>
#include <cstdlib>
#include "csr_sym.hpp"
using namespace lcgh;
int main(int argc, char **argv)
{
    const int inner0 = atoi(argv[1]), S = atoi(argv[2]), G = atoi(argv[3]);
    for (int w = 0; w < S; w++) printf("%d ", sym_group_block_of(w, inner0, S, G));
    printf("\n");
    return 0;
}
"""


def test_every_block_once_and_consecutive_per_xcd(tmp_path):
    src = tmp_path / "sym_group_map.cpp"
    src.write_text(SRC)
    exe = tmp_path / "sym_group_map"
    subprocess.check_call(["g++", "-O1", "-std=c++11", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "liblcg_amd", "csrc"), str(src), "-o", str(exe)])
    for inner0 in (0, 2056):
        for S in list(range(1, 41)) + [63, 64, 65, 127, 128, 200]:
            for G in (1, 2, 4, 8):
                blocks = [int(v) for v in subprocess.check_output([str(exe), str(inner0), str(S), str(G)], text=True).split()]
                assert sorted(blocks) == list(range(inner0, inner0 + S)), (inner0, S, G, blocks)         # every block once
                win = 8 * G
                full = S // win * win
                assert blocks[full:] == list(range(inner0 + full, inner0 + S)), (inner0, S, G)            # the rest in order
                if G == 1:
                    assert blocks == list(range(inner0, inner0 + S))
                for w0 in range(0, full, win):
                    for xcd in range(8):
                        mine = blocks[w0 + xcd:w0 + win:8]                                                 # this XCD's workgroups of the window
                        first = inner0 + w0 + xcd * G
                        assert mine == list(range(first, first + G)), (inner0, S, G, w0, xcd, mine)
