"""Host (no GPU): csrc/gs_sort_key.h, the one statement of the sort key layouts, compiled into a stand-alone program with g++.

The narrow key is the wide key (tile << depth_bits | depth code) without its low byte, in 16 bits.  Checked against plain Python
integers for depth fields of 8, 9, 15 and 16 bits with 24 - depth_bits tile bits (24 key bits: all sixteen of the narrow key in use),
at every corner of (tile, code) and a few thousand seeded pairs: the narrow key and the code's low byte give the wide key back, narrow
keys order as wide >> 8 does, the tile comes back out of the narrow key, the exported key is the reference's (tile << 32) + code; and
the class rule: narrow up to 24 key bits behind the first pass, wide at 25 bits, with 7 depth bits, without the first pass, with
the switch off."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER_DIR = os.path.join(ROOT, "taichi_3d_gaussian_splatting_amd", "csrc")

PROGRAM = r"""
#include "gs_sort_key.h"
#include <cstdio>
int main()
{
    char what;
    while (scanf(" %c", &what) == 1) {
        if (what == 'k') {
            int db; unsigned tile, code;
            if (scanf("%d %u %u", &db, &tile, &code) != 3) return 1;
            const uint16_t n = gs_narrow_key(tile, code, db);
            printf("%u %llu %u %u %lld\n", (unsigned)n, (unsigned long long)gs_wide_key(tile, code, db), gs_wide_of_narrow(n, code),
                   gs_narrow_tile(n, db), (long long)gs_reference_key(gs_narrow_tile(n, db), code));
        } else if (what == 'c') {
            int kb, db, first, allowed;
            if (scanf("%d %d %d %d", &kb, &db, &first, &allowed) != 4) return 1;
            printf("%d %d\n", gs_key_bytes(kb, db, first != 0, allowed != 0), gs_key_dropped_bits(gs_key_bytes(kb, db, first != 0, allowed != 0)));
        } else return 1;
    }
    return 0;
}
"""


@pytest.fixture(scope="module")
def ask(tmp_path_factory):
    d = tmp_path_factory.mktemp("sort_key")
    src, exe = d / "sort_key.cpp", d / "sort_key"
    src.write_text(PROGRAM)
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I", HEADER_DIR, str(src), "-o", str(exe)])

    def run(lines):
        out = subprocess.run([str(exe)], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True).stdout
        rows = [tuple(int(x) for x in ln.split()) for ln in out.splitlines()]
        assert len(rows) == len(lines)
        return rows
    return run


def _pairs(depth_bits):
    """(tile, code) at the corners of both fields and around the byte boundary of the code, then 3000 seeded ones"""
    tile_bits = 24 - depth_bits
    tmax, cmax = (1 << tile_bits) - 1, (1 << depth_bits) - 1
    tiles = sorted({0, 1, tmax // 2, tmax - 1, tmax} & set(range(tmax + 1)))
    codes = sorted({0, 1, 254, 255, 256, 257, 511, 512, cmax // 2, cmax - 256, cmax - 255, cmax - 1, cmax} & set(range(cmax + 1)))
    pairs = [(t, c) for t in tiles for c in codes]
    rng = np.random.default_rng(1000 + depth_bits)
    pairs += list(zip(rng.integers(0, tmax + 1, 3000).tolist(), rng.integers(0, cmax + 1, 3000).tolist()))
    return pairs


@pytest.mark.parametrize("depth_bits", [8, 9, 15, 16])
def test_narrow_key_reassembles_and_orders_as_the_wide_one(ask, depth_bits):
    pairs = _pairs(depth_bits)
    rows = ask(["k %d %d %d" % (depth_bits, t, c) for t, c in pairs])
    wide_ref = np.array([(t << depth_bits) | c for t, c in pairs], np.int64)
    narrow, wide, rebuilt, tile, refkey = (np.array(col, np.int64) for col in zip(*rows))
    assert np.array_equal(wide, wide_ref)
    assert np.array_equal(narrow, wide_ref >> 8) and narrow.max() < 1 << 16
    assert narrow.max() == (1 << 16) - 1                                  # the corner (tmax, cmax) sets all sixteen bits
    assert np.array_equal(rebuilt, wide_ref)                              # narrow key + low byte of the code
    assert np.array_equal(tile, np.array([t for t, _ in pairs]))
    assert np.array_equal(refkey, np.array([(t << 32) + c for t, c in pairs], np.int64))
    # the same order: a stable sort by the narrow key of pairs already stably sorted by the low byte is the sort by the wide key
    by_low = np.argsort(wide_ref & 255, kind="stable")
    two_step = by_low[np.argsort(narrow[by_low], kind="stable")]
    assert np.array_equal(two_step, np.argsort(wide_ref, kind="stable"))
    # and pairwise: narrow keys compare as wide >> 8 does
    a, b = np.arange(len(pairs) - 1), np.arange(1, len(pairs))
    assert np.array_equal(np.sign(narrow[a] - narrow[b]), np.sign((wide_ref[a] >> 8) - (wide_ref[b] >> 8)))


def test_class_rule(ask):
    cases = {                                   # (key_bits, depth_bits, first pass, switch) -> bytes
        (24, 11, 1, 1): 2, (24, 8, 1, 1): 2, (24, 16, 1, 1): 2, (9, 8, 1, 1): 2, (16, 8, 1, 1): 2,
        (25, 12, 1, 1): 4, (25, 17, 1, 1): 4, (32, 16, 1, 1): 4,
        (15, 7, 1, 1): 4, (15, 7, 0, 1): 4,       # 7 depth bits: digit 0 holds a tile bit (the host passes no first pass there either)
        (24, 11, 0, 1): 4,                        # no first pass: nothing has placed the low byte
        (24, 11, 1, 0): 4,                        # the switch
        (33, 20, 1, 1): 8, (40, 31, 0, 1): 8, (33, 20, 1, 0): 8,
    }
    keys = list(cases)
    rows = ask(["c %d %d %d %d" % k for k in keys])
    for k, (nbytes, dropped) in zip(keys, rows):
        assert nbytes == cases[k], k
        assert dropped == (8 if nbytes == 2 else 0), k
