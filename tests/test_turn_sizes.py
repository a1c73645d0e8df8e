"""tests/turn_sizes.py against the sources it restates: the tile, the scan
block and the grid's workgroups per CU, read out of the two files."""
import os
import re

import turn_sizes as TS

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "libquic_amd",
                    "csrc")


def source(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def test_constants_are_the_sources():
    header, kernels = source("qfec_internal.h"), source("qturn_kernels.hip")
    tile = re.findall(r"constexpr\s+uint32_t\s+kReviveTile\s*=\s*(\d+)\s*;", header)
    block = re.findall(r"constexpr\s+int\s+kRvScanBlock\s*=\s*(\d+)\s*;", kernels)
    grid = re.findall(r"inline\s+uint32_t\s+per_packet_grid\s*\([^)]*\)\s*\{[^}]*?"
                      r"\(ncu\s*\?\s*ncu\s*:\s*\d+u\)\s*\*\s*(\d+)u\s*\)", kernels)
    assert [int(x) for x in tile] == [TS.TILE], tile
    assert [int(x) for x in block] == [TS.SCAN_BLOCK], block
    assert [int(x) for x in grid] == [TS.GRID_PER_CU], grid
    # the one-workgroup scan takes a trip per scan block
    assert re.search(r"tile_scan\(uint64_t n[^{]*\{[^}]*t0 \+= kRvScanBlock", kernels)
    assert TS.SCAN_WRAP == TS.TILE * TS.SCAN_BLOCK + 1 and TS.WAVE == 64
