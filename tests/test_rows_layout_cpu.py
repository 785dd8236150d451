"""The byte queries of the MPNN workspaces, pinned across the refactor of the global-row host path.

eco_mpnn_workspace_bytes, eco_mpnn_forward_wg_workspace_bytes (7 and 13 observables),
eco_mpnn_grad_large_workspace_bytes and eco_mpnn_grad_wg_workspace_bytes are pure host functions: they run without a
GPU.  Every N of NS (both sides of 512, 2048 and 8192, and sizes that are no multiple of the 16-row tile) meets every
batch of BATCHES (0, small, and both sides of the 32-bit row index of each range: 65536 x 513, 16377 x 2049,
4096 x 8192 rows exceed (2^31 - 1) / 64).

Provenance of EXPECTED: printed by this file from a library built from commit de5273e, the parent of the refactor that
introduced mpnn_grad_rows_layout, and pasted here unchanged.  To regenerate, build that commit's library and run

    ECO_HIP_LIB=/path/to/parent/libecohip.so python tests/test_rows_layout_cpu.py

which prints the EXPECTED literal below.
"""
import os
import sys

import pytest

NS = (512, 513, 528, 2047, 2048, 2049, 2064, 8191, 8192, 8193)
BATCHES = (0, 1, 2, 64, 4095, 4096, 16376, 16377, 65536)


def _queries():
    from eco_hip import _lib
    lib = _lib.lib
    return {
        "eco_mpnn_workspace_bytes": lib.eco_mpnn_workspace_bytes,
        "eco_mpnn_forward_wg_workspace_bytes/7": lambda n, b: lib.eco_mpnn_forward_wg_workspace_bytes(n, b, 7),
        "eco_mpnn_forward_wg_workspace_bytes/13": lambda n, b: lib.eco_mpnn_forward_wg_workspace_bytes(n, b, 13),
        "eco_mpnn_grad_large_workspace_bytes": lib.eco_mpnn_grad_large_workspace_bytes,
        "eco_mpnn_grad_wg_workspace_bytes": lib.eco_mpnn_grad_wg_workspace_bytes,
    }


# EXPECTED[query][i][j]: the query at (NS[i], BATCHES[j])
EXPECTED = {
    'eco_mpnn_workspace_bytes': [
        [0, 131328, 262400, 8388864, 536740096, 536871168, 2146435328, 2146566400, 8589934848],
        [0, 3796352, 3796352, 35931760, 2195551600, 2195551600, 8772965712, 8775107936, 35104044400],
        [0, 3896108, 3896108, 36969004, 2259536428, 2259536428, 9028665388, 9030871340, 36127230508],
        [0, 33781008, 33781008, 162006048, 8778728736, 8778728736, 35022120256, 35030668592, 140081169696],
        [0, 33785124, 33785124, 162071844, 8782939428, 8782939428, 35038954788, 35047507236, 140148540708],
        [0, 34037888, 34037888, 162388336, 8787658864, 8787658864, 35057084496, 35065641056, 140220352624],
        [0, 34248236, 34248236, 163536172, 8851754284, 8851754284, 35312894764, 35321515052, 141243649324],
        [0, 437125392, 437125392, 950210592, 35429536032, 35429536032, 140440973632, 140475179312, 560828780832],
        [0, 437129508, 437129508, 950276388, 35433746724, 35433746724, 140457808164, 140492017956, 560896151844],
        [0, 438119552, 438119552, 951330160, 35439203440, 35439203440, 140476675152, 140510889056, 560968701040],
    ],
    'eco_mpnn_forward_wg_workspace_bytes/7': [
        [0, 0, 0, 0, 0, 0, 0, 0, 0],
        [0, 0, 0, 0, 0, 0, 0, 0, 0],
        [0, 0, 0, 0, 0, 0, 0, 0, 0],
        [0, 0, 0, 0, 0, 0, 0, 0, 0],
        [0, 0, 0, 0, 0, 0, 0, 0, 0],
        [0, 1585408, 3170560, 101449984, 6491197696, 6492782848, 0, 0, 0],
        [0, 1585408, 3170560, 101449984, 6491197696, 6492782848, 0, 0, 0],
        [0, 6291712, 12583168, 402653440, 25763512576, 0, 0, 0, 0],
        [0, 6291712, 12583168, 402653440, 25763512576, 0, 0, 0, 0],
        [0, 0, 0, 0, 0, 0, 0, 0, 0],
    ],
    'eco_mpnn_forward_wg_workspace_bytes/13': [
        [0, 0, 0, 0, 0, 0, 0, 0, 0],
        [0, 0, 0, 0, 0, 0, 0, 0, 0],
        [0, 0, 0, 0, 0, 0, 0, 0, 0],
        [0, 0, 0, 0, 0, 0, 0, 0, 0],
        [0, 0, 0, 0, 0, 0, 0, 0, 0],
        [0, 1585408, 3170560, 101449984, 6491197696, 6492782848, 0, 0, 0],
        [0, 1585408, 3170560, 101449984, 6491197696, 6492782848, 0, 0, 0],
        [0, 6291712, 12583168, 402653440, 25763512576, 0, 0, 0, 0],
        [0, 6291712, 12583168, 402653440, 25763512576, 0, 0, 0, 0],
        [0, 0, 0, 0, 0, 0, 0, 0, 0],
    ],
    'eco_mpnn_grad_large_workspace_bytes': [
        [0, 0, 0, 0, 0, 0, 0, 0, 0],
        [0, 45506304, 49069056, 269959680, 14631429120, 14634991872, 58385635584, 58389198336, 0],
        [0, 45594624, 49245696, 275612160, 14993099520, 14996750592, 59831963904, 59835614976, 0],
        [0, 56094976, 70246400, 947634688, 57992040960, 58006192384, 231785728256, 231799879680, 0],
        [0, 56100864, 70258176, 948011520, 58016152320, 58030309632, 231882150144, 231896307456, 0],
        [0, 0, 0, 0, 0, 0, 0, 0, 0],
        [0, 0, 0, 0, 0, 0, 0, 0, 0],
        [0, 0, 0, 0, 0, 0, 0, 0, 0],
        [0, 0, 0, 0, 0, 0, 0, 0, 0],
        [0, 0, 0, 0, 0, 0, 0, 0, 0],
    ],
    'eco_mpnn_grad_wg_workspace_bytes': [
        [0, 0, 0, 0, 0, 0, 0, 0, 0],
        [0, 0, 0, 0, 0, 0, 0, 0, 0],
        [0, 0, 0, 0, 0, 0, 0, 0, 0],
        [0, 0, 0, 0, 0, 0, 0, 0, 0],
        [0, 0, 0, 0, 0, 0, 0, 0, 0],
        [0, 56123136, 70302720, 949436928, 58107356160, 58121535744, 232246876416, 0, 0],
        [0, 56211456, 70479360, 955089408, 58469026560, 58483294464, 0, 0, 0],
        [0, 98562304, 155181056, 3665543680, 231895749120, 231952367872, 0, 0, 0],
        [0, 98568192, 155192832, 3665920512, 231919860480, 0, 0, 0, 0],
        [0, 0, 0, 0, 0, 0, 0, 0, 0],
    ],
}


@pytest.mark.parametrize("name", list(EXPECTED))
def test_byte_queries_match_the_parent(name):
    q = _queries()[name]
    assert len(EXPECTED[name]) == len(NS) and all(len(row) == len(BATCHES) for row in EXPECTED[name])
    got = [[q(n, b) for b in BATCHES] for n in NS]
    bad = [(n, b, got[i][j], EXPECTED[name][i][j]) for i, n in enumerate(NS) for j, b in enumerate(BATCHES)
           if got[i][j] != EXPECTED[name][i][j]]
    assert not bad, (name, bad)


def test_table_covers_the_five_queries_and_both_sides_of_every_bound():
    assert sorted(EXPECTED) == sorted(_queries())
    large, wg = EXPECTED["eco_mpnn_grad_large_workspace_bytes"], EXPECTED["eco_mpnn_grad_wg_workspace_bytes"]
    for i, n in enumerate(NS):
        for j, b in enumerate(BATCHES):
            in_large = 512 < n <= 2048 and b >= 1 and n * b <= (2 ** 31 - 1) // 64
            in_wg = 2048 < n <= 8192 and b >= 1 and n * b <= (2 ** 31 - 1) // 64
            assert (large[i][j] > 0) == in_large and (wg[i][j] > 0) == in_wg, (n, b)


if __name__ == "__main__":
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path.insert(0, os.path.join(os.path.dirname(here), "eco-dqn_amd"))
    print("EXPECTED = {")
    for name, q in _queries().items():
        print(f"    {name!r}: [")
        for n in NS:
            print("        [" + ", ".join(str(q(n, b)) for b in BATCHES) + "],")
        print("    ],")
    print("}")
