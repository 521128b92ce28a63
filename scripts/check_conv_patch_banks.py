"""Dev check: LDS layout of conv_patch.hip.h (round 3: dz-pure fragments, row pitch 4128 / 2080 bytes) is bank-conflict free
for every ds_read_b128 of its K loop.  Fragment = column pair f of the tile's two pooled rows: rows 0-3 = (row 0, col 2f),
4-7 = (row 1, col 2f), 8-11 = (row 1, col 2f+1), 12-15 = (row 0, col 2f+1); row e of a window = (dy, dx); LDS byte address
= (2 ypl + dy + ky) LP + (2 xp + dx + kx) 64 + 16 fk."""
GROUPS = [list(range(0, 4)) + list(range(12, 16)) + list(range(20, 28)),
          list(range(4, 12)) + list(range(16, 20)) + list(range(28, 32)),
          list(range(32, 36)) + list(range(44, 48)) + list(range(52, 60)),
          list(range(36, 44)) + list(range(48, 52)) + list(range(60, 64))]
COMP = [(0, 0), (1, 0), (1, 1), (0, 1)]


def main():
    for name, lp, pairs in (('56 x 56 planes (conv2a)', 4128, 14), ('28 x 28 planes (conv3a, conv3b)', 2080, 7)):
        extra, reads = 0, 0
        for f in range(pairs):
            for ky in range(3):
                for kx in range(3):
                    for g in GROUPS:
                        slots = {}
                        for lane in g:
                            frow, fk = lane & 15, lane >> 4
                            ypl, xo = COMP[frow >> 2]
                            dy, dx = (frow >> 1) & 1, frow & 1
                            addr = (2 * ypl + dy + ky) * lp + (2 * (2 * f + xo) + dx + kx) * 64 + fk * 16
                            slots.setdefault((addr % 256) // 16, set()).add(addr)
                        reads += 1
                        extra += sum(len(v) - 1 for v in slots.values())
        print('conv_patch, %s: %d group reads, %d extra LDS cycles' % (name, reads, extra))
        assert extra == 0
    pure()
    return 0


def pure():
    """Plane-pure form (conv3a / conv3b inference forward): two plane buffers of 12 rows (stride 25 088), M wave m reads the rows
    of clip window 2 q + m at + 6 m rows, accumulator slot i = columns 4 i .. 4 i + 3 at + 256 i: fragment base
    = buf 25088 + (6 m + 2 ypl + dy) LP + (2 xo + dx) 64 + 16 fk, immediates 256 i + ky LP + 64 kx.  Also checked: every read
    stays inside the 30 pixels of its row and the 12 rows of its buffer, and the 24 DMA instructions of a plane (row j / 2,
    part j % 2, 1 KB each) tile the buffer rows without overlap."""
    lp, stride = 2080, 25088
    extra, reads = 0, 0
    for buf in range(2):
        for m in range(2):
            for i in range(7):
                for ky in range(3):
                    for kx in range(3):
                        for g in GROUPS:
                            slots = {}
                            for lane in g:
                                frow, fk = lane & 15, lane >> 4
                                ypl, xo = COMP[frow >> 2]
                                dy, dx = (frow >> 1) & 1, frow & 1
                                row, pix = 6 * m + 2 * ypl + dy + ky, 4 * i + 2 * xo + dx + kx
                                assert 6 * m <= row < 6 * m + 6 and 0 <= pix < 30
                                addr = buf * stride + (6 * m + 2 * ypl + dy) * lp + (2 * xo + dx) * 64 + fk * 16 + 256 * i + ky * lp + kx * 64
                                assert addr == buf * stride + row * lp + pix * 64 + fk * 16 and addr + 16 <= (buf + 1) * stride
                                slots.setdefault((addr % 256) // 16, set()).add(addr)
                            reads += 1
                            extra += sum(len(v) - 1 for v in slots.values())
    dst = sorted((j >> 1) * lp + (j & 1) * 1024 for j in range(24))
    assert all(b - a >= 1024 for a, b in zip(dst, dst[1:])) and dst[-1] + 1024 <= stride and 2 * stride == 50176
    print('conv_patch, plane-pure form (conv3a, conv3b inference): %d group reads, %d extra LDS cycles' % (reads, extra))
    assert extra == 0


if __name__ == '__main__':
    raise SystemExit(main())
