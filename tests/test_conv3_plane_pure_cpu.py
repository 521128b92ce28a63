"""CPU model of the tile walk of conv_patch_pure_body (csrc/conv_patch.hip.h): the plane-pure form of conv3a / conv3b.

The functions below restate, line by line, the index arithmetic of the kernel: tile_of(), decode() (conv3a: z-adjacent,
rotated; conv3b: chunks of 16 pairs), the executed tap groups of a pass, and what every executed step issues ahead -- the
filter slab three executed steps on and, in the first step of a tap group, the plane of the next executed tap group."""
import itertools

import pytest

NPC = 16                      # RGP_CP_CHUNK28P
YT = 7
GRID = 256                    # workgroups of a launch (one per CU)


class Layer:
    def __init__(self, pool):
        self.pool = pool
        self.ncc = 8 if pool else 4               # channel sweeps of 32: conv3b 256, conv3a 128 input channels
        self.zt = 4 if pool else 8
        self.npass = 2 if pool else 1
        self.tpp = self.zt * YT


def tile_of(t, nt):
    q, r, x, y = nt >> 3, nt & 7, t & 7, t >> 3
    return (x * (q + 1) if x < r else r * (q + 1) + (x - r) * q) + y


def decode(layer, tile, npair):
    if not layer.pool:                            # conv3a: (pair, yp, z + rotation by the tile's block of 32)
        q, r = divmod(tile, layer.tpp)
        return q, ((r % layer.zt) + (tile >> 5)) & (layer.zt - 1), r // layer.zt
    c, r = divmod(tile, NPC * layer.tpp)          # conv3b: (chunk, zp, pair, yp)
    cp = min(NPC, npair - c * NPC)
    zt, r2 = divmod(r, cp * YT)
    w, yp = divmod(r2, YT)
    return c * NPC + w, zt, yp


def tiles_of_block(layer, n, block, grid):
    npair = (n + 1) >> 1
    nt = npair * layer.tpp
    return [decode(layer, tile_of(t, nt), npair) for t in range(block, nt, grid)]


def groups_of(z):
    return (1 if z == 0 else 0), (1 if z == 7 else 2)


def walk(layer, tiles):
    """The kernel's loops over one workgroup's tiles: per executed step what it multiplies and what it issues."""
    executed, issued, fetched, read_plane, stores, kinds = [], [], [], [], [], []
    buf = 0
    for ti, (q, zt, yp) in enumerate(tiles):
        qn, ztn, ypn = tiles[ti + 1] if ti + 1 < len(tiles) else tiles[ti]
        for ps in range(layer.npass):
            z = 2 * zt + ps if layer.pool else zt
            k0, k1 = groups_of(z)
            same_tile = ps + 1 < layer.npass
            jq, jyp = (q, yp) if same_tile else (qn, ypn)
            jz = z + 1 if same_tile else (2 * ztn if layer.pool else ztn)
            jk0 = groups_of(jz)[0]
            kinds.append((k1 - k0 + 1, zt))
            for cc in range(layer.ncc):
                for kz in range(k0, k1 + 1):
                    if kz < k1:
                        ncc, nkz, npl = cc, kz + 1, (q, z + kz + 1, yp, cc)
                    elif cc + 1 < layer.ncc:
                        ncc, nkz, npl = cc + 1, k0, (q, z + k0, yp, cc + 1)
                    else:
                        ncc, nkz, npl = 0, jk0, (jq, jz + jk0, jyp, 0)
                    read_plane.append(((q, z + kz, yp, cc), buf))
                    fetched.append((npl, buf ^ 1))
                    for t9 in range(9):
                        executed.append((cc, kz * 9 + t9))
                        issued.append((cc, kz * 9 + t9 + 3) if t9 < 6 else (ncc, nkz * 9 + t9 - 6))
                    buf ^= 1
            stores.append((q, z, yp))
    return executed, issued, fetched, read_plane, stores, kinds


@pytest.mark.parametrize('pool', [False, True])
def test_every_window_plane_band_is_produced_exactly_once(pool):
    layer = Layer(pool)
    for n in range(1, 41):
        npair = (n + 1) >> 1
        nt = npair * layer.tpp
        assert sorted(tile_of(t, nt) for t in range(nt)) == list(range(nt))
        seen = {}
        for block in range(min(GRID, nt)):
            for q, zt, yp in tiles_of_block(layer, n, block, GRID):
                assert 0 <= q < npair and 0 <= zt < layer.zt and 0 <= yp < YT
                for ps in range(layer.npass):
                    z = 2 * zt + ps if pool else zt
                    for m in (0, 1):
                        w = 2 * q + m
                        if w < n:                  # the kernel's store guard: the second window of a ragged pair stores nothing
                            seen[(w, z, yp)] = seen.get((w, z, yp), 0) + 1
        assert all(w < n for w, _, _ in seen)
        assert set(seen) == set(itertools.product(range(n), range(8), range(YT))), n
        assert set(seen.values()) == {1}, n


@pytest.mark.parametrize('pool', [False, True])
@pytest.mark.parametrize('n,grid', [(1, 1), (3, 2), (19, 5), (40, 7)])
def test_look_ahead_is_the_executed_sequence_shifted_by_three_steps(pool, n, grid):
    """A small grid gives every workgroup a long walk: all pass-type transitions occur (asserted below)."""
    layer = Layer(pool)
    trans = set()
    for block in range(grid):
        tiles = tiles_of_block(layer, n, block, grid)
        executed, issued, fetched, read_plane, stores, kinds = walk(layer, tiles)
        # slabs 0 .. 2 come from the prologue; step i issues the slab of step i + 3
        assert issued[:len(executed) - 3] == executed[3:]
        # an executed tap group multiplies the plane its predecessor fetched, out of the buffer it was fetched into, and no
        # halo plane (0 or 9 of the halo-padded input) is ever read
        assert fetched[:-1] == read_plane[1:]
        assert read_plane[0][1] == 0 and all(1 <= pl[1] <= 8 for pl, _ in read_plane)
        assert len(set(stores)) == len(stores)
        for (a, za), (b, zb) in zip(kinds, kinds[1:]):
            trans.add((a, b))
            if za != zb:
                trans.add('z')
    if n >= 19:
        assert {(2, 3), (3, 2), (3, 3), 'z'} <= trans, trans
