"""The sizes at which a receive-turn pass takes a second trip of one of its two
loops (libquic_amd/csrc/qturn_kernels.hip), for the tests that run every call
past them.  tests/test_turn_sizes.py pins the constants to the sources.

The one-workgroup scan (tile_scan) takes a trip per SCAN_BLOCK elements and
carries its base from trip to trip: a scan over tiles of TILE items takes its
second trip at SCAN_WRAP items, acks_scan_kernel at SCAN_BLOCK + 1 acks.

The capped grid (per_packet_grid) launches at most ncu * GRID_PER_CU
workgroups of TILE lanes, which loop: a kernel of one lane per item takes its
second trip at grid_wrap() items, one of a wave per item (acks_walk_kernel,
ack_write_kernel, record_raise_kernel) at wave_wrap() items.

Left out: record_advance_kernel and frames_set_kernel loop over connections,
a lane each; their second trip needs more than ncu * 16 * 256 connections (2^20
at 256 CUs, 64 MiB of cells at the smallest window), and no test goes there.
"""
TILE = 256         # kReviveTile: items per workgroup trip
SCAN_BLOCK = 1024  # kRvScanBlock: elements per trip of the one-workgroup scan
GRID_PER_CU = 16   # per_packet_grid: workgroups per CU
WAVE = 64
SCAN_WRAP = TILE * SCAN_BLOCK + 1


def ncu():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def grid_wrap():
    """one item more than a full grid of tiles: the first workgroup's second trip"""
    return ncu() * GRID_PER_CU * TILE + 1


def wave_wrap():
    """one item more than a full grid of waves, for the kernels of a wave per item"""
    return ncu() * GRID_PER_CU * TILE // WAVE + 1
