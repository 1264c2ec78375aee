"""Shapes at which the persistent blocks of the 3x3 split kernels own more than one tile (shared by the GPU test modules)."""


def multi_tile_cout(spatial):
    """Cout at which a 3x3 split launch over `spatial` tiles of 16 rows x 32 pixels gives its persistent blocks MORE THAN ONE tile each,
    unevenly: the launch has blocks = 8 (n_cu // 8) blocks and T = spatial * Cout / 64 tiles; the smallest T that is a multiple of 27
    with blocks < T < 2 blocks and T % 8 != 0 (270 on 256 CUs) -- some blocks walk two tiles, some one, and the eight XCD ranges of the
    tile list differ in length.  What only shows there: the staging state crossing a tile boundary, the chunk-buffer parity and the
    statistics scratch of a second tile."""
    from onet_amd import ops
    blocks = 8 * (ops.n_cu() // 8)
    T = 27 * (blocks // 27 + 1)
    while T % 8 == 0:
        T += 27
    assert T % spatial == 0 and blocks < T < 2 * blocks and T % 8 != 0, (T, spatial, blocks)
    return 64 * (T // spatial)
