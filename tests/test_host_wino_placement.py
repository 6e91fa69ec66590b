"""Host-side checks (no GPU) of where the persistent Winograd kernels put their work: tmf_xcd_slot — the library's one placement
rule (xcd_contiguous, csrc/tmf_common.h), which conv3d_winox_kernel and conv3d_wino_p_kernel apply to their workgroup index and
conv3d_wino_wgrad_p_kernel to its split — and tmf_conv3d_wino_grid, the workgroups of a launch's first window."""
import pytest

GRIDS = range(1, 305)                 # every grid a device of up to 304 compute units can get


def _slots(lib, grid):
    return [lib.tmf_xcd_slot(b, grid) for b in range(grid)]


def test_xcd_slot_is_a_permutation_with_one_contiguous_range_per_xcd():
    """Workgroup b runs on XCD b % 8.  For EVERY grid — not only the multiples of 8 — block -> slot is a permutation of
    0 .. grid - 1, the blocks of one XCD hold one contiguous ascending range of grid // 8 slots (the first grid % 8 XCDs one
    more), and the ranges follow each other in XCD order."""
    from transmf_ad_amd import _lib
    lib = _lib.load()
    for grid in GRIDS:
        slots = _slots(lib, grid)
        assert sorted(slots) == list(range(grid)), grid
        nxt = 0
        for xcd in range(8):
            mine = [slots[b] for b in range(xcd, grid, 8)]
            assert len(mine) == grid // 8 + (1 if xcd < grid % 8 else 0), (grid, xcd)
            assert mine == list(range(nxt, nxt + len(mine))), (grid, xcd)
            nxt += len(mine)
        assert nxt == grid
        assert lib.tmf_xcd_slot(-1, grid) == -1 and lib.tmf_xcd_slot(grid, grid) == -1
    assert lib.tmf_xcd_slot(0, 0) == -1
    # a multiple of 8 keeps the placement these kernels had before the rule covered every grid
    for grid in (8, 16, 216, 256):
        assert _slots(lib, grid) == [(b & 7) * (grid >> 3) + (b >> 3) for b in range(grid)]


def _rounds_grid(n, ncu):
    """min(n, ncu), evened to the rounds the window needs — the rule the statistic rows are promised under: rows at and past
    this count are zeros (tmf_conv3d_wino_stat_blocks rows in all)"""
    if n <= ncu:
        return n
    rounds = -(-n // ncu)
    return -(-n // rounds)


# B, D, H, W: the volumes whose item lists must be covered (ragged, transposed, one brick row, the benchmark's 48^3)
VOLUMES = [(2, 22, 27, 22), (3, 15, 21, 9), (1, 8, 4, 8), (8, 48, 48, 48)]


@pytest.mark.parametrize("cap", [0, 5, 7, 16, 100], ids=lambda c: f"cus{c}")
def test_every_item_has_exactly_one_workgroup_and_round(cap):
    """The launch's grid (tmf_conv3d_wino_grid) and the placement rule together: over the workgroups b and their rounds i, the
    items slot(b) + i * grid below the window's count are every item exactly once — for 1, 2, 3, 4 and 8 groups of output
    channels, the split kernel's launches (cin % 32 == 0) and the fp32 kernel's (cin = 8), at the device's workgroup count and
    capped ("wino_cus"); the grid is the rounds-sized one and never exceeds the statistic rows."""
    from transmf_ad_amd import _lib
    lib = _lib.load()
    assert lib.tmf_set_option(b"wino_cus", cap) == 0
    try:
        for B, D, H, W in VOLUMES:
            ncu = lib.tmf_conv3d_wino_stat_blocks(B, D, H, W)
            assert ncu == cap or (cap == 0 and ncu >= 64)
            for cin in (32, 8):
                for groups in (1, 2, 3, 4, 8):
                    cout = 32 * groups
                    kernel = lib.tmf_conv3d_wino_kernel_name2(B, D, H, W, cin, cout, 1)
                    tab = 256 if kernel.startswith(b"conv3d_winox") else (448 if kernel.endswith(b", 1>") else 768)
                    items = lib.tmf_conv3d_wino_bricks2(B, D, H, W, cin, cout) * groups
                    n = min(items, ncu * tab)                               # the first window
                    grid = lib.tmf_conv3d_wino_grid(B, D, H, W, cin, cout)
                    assert grid == _rounds_grid(n, ncu) and 1 <= grid <= ncu, (B, D, H, W, cin, cout)
                    seen = [0] * n
                    for b in range(grid):
                        for item in range(lib.tmf_xcd_slot(b, grid), n, grid):
                            seen[item] += 1
                    assert seen == [1] * n, (B, D, H, W, cin, cout)
                    # every workgroup has work, and their loads differ by at most one item
                    loads = [len(range(lib.tmf_xcd_slot(b, grid), n, grid)) for b in range(grid)]
                    assert min(loads) >= 1 and max(loads) - min(loads) <= 1
    finally:
        assert lib.tmf_set_option(b"wino_cus", 0) == 0


def test_wino_grid_at_the_benchmark_shape_and_its_refusals():
    """The eight split-kernel launches of an encoder at B = 8, 96^3 on 256 compute units: four of them get 247 workgroups, no
    multiple of 8 — the grids the placement rule has to cover.  No grid without a persistent launch."""
    from transmf_ad_amd import _lib
    lib = _lib.load()
    assert lib.tmf_set_option(b"wino_cus", 256) == 0
    try:
        if lib.tmf_conv3d_wino_stat_blocks(8, 48, 48, 48) == 256:           # (a cap never raises the count above the device's)
            grid = lambda v, ci, co: lib.tmf_conv3d_wino_grid(8, v, v, v, ci, co)         # noqa: E731
            assert grid(48, 32, 32) == 247 and grid(48, 64, 32) == 247 and grid(24, 64, 128) == 247
            assert grid(48, 32, 64) == 256 and grid(24, 64, 64) == 216 and grid(24, 128, 64) == 216
    finally:
        assert lib.tmf_set_option(b"wino_cus", 0) == 0
    assert lib.tmf_conv3d_wino_grid(0, 4, 4, 4, 32, 32) == 0 and lib.tmf_conv3d_wino_grid(1, 4, 8, 8, 32, 48) == 0
    assert lib.tmf_set_option(b"wino_p", 0) == 0
    try:
        assert lib.tmf_conv3d_wino_grid(8, 48, 48, 48, 32, 32) == 0
    finally:
        assert lib.tmf_set_option(b"wino_p", 1) == 0
