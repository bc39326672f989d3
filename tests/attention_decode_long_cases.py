"""What the tests of vidil_attention's key-split form (kv_tiled = 2: attn_dsplit_kernel in csrc/attention.hip) share: the
kernel's slicing of a unit's key tiles, mirrored, and the keys a one-hot row is aimed at."""

NW = 4                        # waves per (kv batch, head) workgroup: launch_dsplit<T, 4> in csrc/attention.hip
TILE = 32                     # keys per fragment tile
LONG_KEYS = 768               # up to here kv_tiled = 2 is dispatched as kv_tiled = 1
MAX_KEYS = 16384


def slice_tiles(Nk, nw=NW):
    """[(first tile, one past the last tile)] of wave 0 .. nw-1: ceil(Nk / 32) tiles cut into nw contiguous slices, wave w
    owning tiles [w * n / nw, (w + 1) * n / nw) — balanced to +-1 tile."""
    n = (Nk + TILE - 1) // TILE
    return [(w * n // nw, (w + 1) * n // nw) for w in range(nw)]


def slice_keys(Nk, nw=NW):
    """The first key of every slice but the first: the boundaries between the waves' slices."""
    return [t0 * TILE for t0, _ in slice_tiles(Nk, nw)[1:]]


def targets(Nk):
    """Keys a one-hot row is aimed at: both ends, 767 / 768 (where the short kernels end), the last partial 16-key block, the
    last partial 32-key tile, and both sides of EVERY boundary between the waves' slices."""
    t = {0, Nk - 1, max(0, Nk - 2), (Nk - 1) // 16 * 16, (Nk - 1) // TILE * TILE}
    t |= {x for x in (767, 768) if x < Nk}
    for k0 in slice_keys(Nk):
        t |= {x for x in (k0 - 1, k0, k0 + 1) if 0 <= x < Nk}
    return sorted(t)
