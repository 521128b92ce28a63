"""Dev check of conv2a's inference forward (conv_patch_bf16_kernel / conv_patch_slab_bf16_kernel<64,128,56,16>: one body,
conv_patch.hip.h), by enumeration:

1. LDS layout.  Models the plane fetch (24 LDS-DMA instructions per plane: 4 per slab row, 16 pixels each -- the last one
   of a row runs 6 pixels into the next row), the fragment bases ra_lo / ra_hi of every wave and the immediates of all 27
   taps, and asserts that
   * every byte a fragment read touches was written by the fetch and holds the pixel / channel chunk the tap wants
     (never one of the 6 pixels beyond the row),
   * the 16 lanes of every ds_read_b128 lane group hit 16 different 16-byte slots (no bank conflict),
   * the four plane buffers stay below the filter ring.
2. Tile order.  A pure-Python model of the kernel's tile_of() / decode() for 56 x 56 planes: every (window, zp, yp) exactly
   once for any window count, and the two properties the order exists for (see check_order()).

Constants mirror PatchCfg<64, 128, 56, 16, true>."""
WP, RPI, LP = 58, 4, 4 * 1024 + 32
PLANE_STRIDE = (6 * LP + 255) // 256 * 256
BRING_OFF = (4 * PLANE_STRIDE + 1023) // 1024 * 1024
YT, ZPN, TPW = 14, 8, 112
GROUPS = [list(range(0, 4)) + list(range(12, 16)) + list(range(20, 28)),
          list(range(4, 12)) + list(range(16, 20)) + list(range(28, 32)),
          list(range(32, 36)) + list(range(44, 48)) + list(range(52, 60)),
          list(range(36, 44)) + list(range(48, 52)) + list(range(60, 64))]


def fetch_map():
    """LDS byte address of a 16-byte chunk -> (plane buffer, slab row, pixel, channel chunk) as the fetch writes it (pixel >= 58: the next row's first pixels, never read)"""
    m = {}
    for k in range(4):
        for j in range(6 * RPI):                             # job j: wave j // 3, instruction j % 3
            r, q = divmod(j, RPI)
            for lane in range(64):
                addr = k * PLANE_STRIDE + r * LP + q * 1024 + lane * 16
                assert addr not in m and addr + 16 <= BRING_OFF
                m[addr] = (k, r, q * 16 + (lane >> 2), lane & 3)
    return m


def check_layout():
    m = fetch_map()
    assert len(m) == 4 * 6 * 64 * 4
    reads = extra = 0
    for wm in range(4):
        wmm, wmh = wm & 1, wm >> 1
        for i in range(7):
            dz = wmm if i < 4 else 1 - wmm
            pair = 7 * wmh + (3 * wmm + i if i < 4 else 4 * wmm + i - 4)
            first = 7 * wmh + (3 * wmm if i < 4 else 4 * wmm)
            for kz in range(3):
                for ky in range(3):
                    for kx in range(3):
                        imm = ky * LP + kx * 64 + (pair - first) * 256
                        for g in GROUPS:
                            slots = set()
                            for lane in g:
                                frow, fk = lane & 15, lane >> 4
                                w = frow >> 2
                                ypl, xo = (1 if w in (1, 2) else 0), w >> 1
                                dy, dx = (frow >> 1) & 1, frow & 1
                                base = (2 * ypl + dy) * LP + (2 * xo + dx) * 64 + fk * 16
                                addr = base + first * 256 + (dz + kz) * PLANE_STRIDE + imm
                                want = (dz + kz, 2 * ypl + dy + ky, 2 * (2 * pair + xo) + dx + kx, fk)
                                assert want[2] < WP and m.get(addr) == want, (wm, i, kz, ky, kx, lane, addr, m.get(addr), want)
                                slots.add((addr % 256) // 16)
                            reads += 1
                            extra += 16 - len(slots)
    print('conv2a, row-wise fetch: %d chunks per 4 planes, %d group reads, %d extra LDS cycles' % (len(m), reads, extra))
    assert extra == 0


def tile_of(t, nt):
    """persistent walk: position t (workgroup id + k * grid) -> tile; XCD t & 7 owns a contiguous range"""
    q, r, x, y = nt >> 3, nt & 7, t & 7, t >> 3
    return (x * (q + 1) if x < r else r * (q + 1) + (x - r) * q) + y


def decode(tile):
    """tile -> (window, zp, yp): the 8 pooled planes of a row pair adjacent, zp rotated by the tile's block of 32"""
    tn, r = divmod(tile, TPW)
    return tn, ((r & 7) + (tile >> 5)) & 7, r >> 3


def check_order(n):
    nt = n * TPW
    seen = [decode(t) for t in range(nt)]
    assert sorted(seen) == [(w, z, y) for w in range(n) for z in range(ZPN) for y in range(YT)], n
    pos = {v: t for t, v in enumerate(seen)}
    # (a) neighbours stay close in the numbering (a lockstep round of an XCD is 32 consecutive tiles of its range): the
    # planes zp, zp + 1 of a row pair are at most 7 tiles apart, the row pairs yp, yp + 1 of a plane at most 15; where the
    # range of an XCD starts at a multiple of 32 (1024 windows: all 8) zp-neighbours are ALWAYS in one round and
    # yp-neighbours whenever both lie in one block of 32
    for (w, z, y), t in pos.items():
        if z + 1 < ZPN:
            assert abs(pos[(w, z + 1, y)] - t) <= 7 and pos[(w, z + 1, y)] >> 5 == t >> 5
        if y + 1 < YT:
            t2 = pos[(w, z, y + 1)]
            assert abs(t2 - t) <= 15 and (t2 - t == 8 or t2 >> 5 != t >> 5)
    # (b) CU i of an XCD meets positions i, i + 32, ... of the XCD's range: over any 8 consecutive rounds it gets every
    # pooled plane once, so exactly two short tiles (zp = 0 and zp = 7)
    q, r = nt >> 3, nt & 7
    for x in range(8):
        start, length = tile_of(x, nt), q + (1 if x < r else 0)
        assert [tile_of(x + 8 * y, nt) for y in range(length)] == list(range(start, start + length))
        for i in range(min(32, length)):
            zs = [decode(start + y)[1] for y in range(i, length, 32)]
            for k in range(len(zs) - 7):
                assert sorted(zs[k:k + 8]) == list(range(8)), (n, x, i, k)
    return True


def main():
    check_layout()
    for n in list(range(1, 41)) + [1024]:
        check_order(n)
    print('conv2a tile order: n = 1 .. 40, 1024: every tile once, neighbours within a round, 2 short tiles per CU and 8 rounds')
    return 0


if __name__ == '__main__':
    raise SystemExit(main())
