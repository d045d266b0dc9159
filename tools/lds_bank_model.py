#!/usr/bin/env python3
"""Brute-force LDS bank-conflict model for the trunk kernels' ds_read_b128 fragment reads.

Model (MI355X_MICROARCH.md, LDS): a wave64 ds_read_b128 is serviced in 4 lane groups
{0-3,12-15,20-27}, {4-11,16-19,28-31}, {32-35,44-47,52-59}, {36-43,48-51,60-63}; bank of byte address a is
(a/4) % 64; identical addresses broadcast; each extra distinct address on a bank adds one cycle.
Prints the average LDS cycles per read over all taps / tiles / k-steps (4.0 = conflict-free); for the Winograd trunk
(k_trunk_w) also the epilogue's 8-byte stores (ds_write_b64: 4 x 16 contiguous lanes, bank = (a/4) % 32), for the board-half
and the row-parity assignment of rows to N-tiles.
The measured SQ_LDS_BANK_CONFLICT agrees with this model (profiles/r01_trunk_pmc.txt)."""
GROUPS = [list(range(0, 4)) + list(range(12, 16)) + list(range(20, 28)),
          list(range(4, 12)) + list(range(16, 20)) + list(range(28, 32)),
          list(range(32, 36)) + list(range(44, 48)) + list(range(52, 60)),
          list(range(36, 44)) + list(range(48, 52)) + list(range(60, 64))]
ZERO = 131072


def key32(xs, ys):
    return (xs & 7) | ((ys & 1) << 3)


def key16(xs, p):
    p, x = p & 1, xs & 7
    return p | ((x & 3) << 1) | ((((x >> 2) & 1) ^ p) << 3)


def addr16(lane, t, tap, kk, key):
    """16x16x32 kernel: tile t = board row t&7 of position pair t>>3; lane c16 = (position bit, column)."""
    g4, c16 = lane >> 4, lane & 15
    pz, cx = c16 >> 3, c16 & 7
    dy, dx = tap // 3 - 1, tap % 3 - 1
    ys, xs = (t & 7) + dy, cx + dx
    ok = 0 <= xs < 8 and 0 <= ys < 8       # tiles with ys off the board are skipped by the kernel
    base = ((2 * (t >> 3) + pz) * 64 + ys * 8 + xs) * 512 if ok else ZERO
    return base | (((kk << 2) ^ g4 ^ key(xs, pz)) << 4)


def addr32(lane, t, tap, kk, key):
    h, r = lane >> 5, lane & 31
    dy, dx = tap // 3 - 1, tap % 3 - 1
    yo, xs = (r >> 3) + dy, (r & 7) + dx
    ys = (t & 1) * 4 + yo
    ok = 0 <= xs < 8 and 0 <= ys < 8
    base = ((t >> 1) * 64 + ys * 8 + xs) * 512 if ok else ZERO
    return base | (((kk << 1) ^ h ^ key(xs, yo)) << 4)


def cycles(addrs):
    tot = 0
    for g in GROUPS:
        banks = {}
        for lane in g:
            a = addrs[lane]
            for b in range(4):
                banks.setdefault(((a // 4) + b) % 64, set()).add(a + 4 * b)
        tot += max(len(v) for v in banks.values())
    return tot


# ---- k_trunk_w (net_wino.hip): the Winograd operand V = [position][tile = row*4 + j][xi][hi 256 B | lo 256 B], its 16-byte
# chunks XOR-ed with a 4-bit key of the tile.  Tile and xi offsets are multiples of 256 B, so a lane's bank is chunk ^ key alone.
#   mapping "halves" (until the row-sharing loop): an N-tile is a board half, lane c = row4*4 + j holds row 4*h + row4; the
#            key is tile & 15 = (row & 3)*4 + j; the six (half, row tap) fragments of a position are rows 4*h + row4 + dy;
#   mapping "parity" (shipped): an N-tile is the even or the odd rows, the lane holds row 2*row4 + parity; the key is
#            (row >> 1)*4 + j; the four fragments F0..F3 of a position are rows 2*row4 + f - 1.
WINO_TILE = 512
WINO_MAPPINGS = ("halves", "parity")
WRITE_GROUPS = [list(range(16 * g, 16 * g + 16)) for g in range(4)]   # ds_write_b64: 4 x 16 contiguous lanes


def wino_key(mapping, y, j):
    return ((((y & 3) if mapping == "halves" else (y >> 1)) * 4) + j) & 15


def wino_row(mapping, row4, sel):
    """board row of a lane: sel = board half (halves) or row parity (parity)"""
    return 4 * sel + row4 if mapping == "halves" else 2 * row4 + sel


def wino_fragments(mapping):
    """the operand fragments a position reads per (k-step, xi): (row offset added to a lane's own row selector, ...) as a list
    of functions row4 -> board row"""
    if mapping == "halves":
        return [(lambda r, h=h, d=d: 4 * h + r + d) for h in (0, 1) for d in (-1, 0, 1)]
    return [(lambda r, f=f: 2 * r + f - 1) for f in range(4)]


def wino_read_addr(mapping, lane, p, frag, kk, xi, half=0):
    """byte address of a lane's ds_read_b128 of fragment `frag` (an entry of wino_fragments), k-step kk, tap xi, hi / lo half"""
    g4, c = lane >> 4, lane & 15
    row4, j = c >> 2, c & 3
    y = frag(row4)
    base = (p * 32 + y * 4 + j) * 4 * WINO_TILE if 0 <= y < 8 else ZERO
    return base + (((kk * 4 + g4) ^ wino_key(mapping, y, j)) << 4) + xi * WINO_TILE + half * 256


def wino_store_addr(mapping, lane, wave, p, sel, xi, half=0):
    """byte address of a lane's 8-byte epilogue store: wave = 16 output channels, lane (g4, c) = channels 16*wave + 4*g4 .. + 3 of
    tile (row(c, sel), j)"""
    g4, c = lane >> 4, lane & 15
    row4, j = c >> 2, c & 3
    y = wino_row(mapping, row4, sel)
    chunk = 2 * wave + (g4 >> 1)
    return (p * 32 + y * 4 + j) * 4 * WINO_TILE + ((chunk ^ wino_key(mapping, y, j)) << 4) + 8 * (g4 & 1) + xi * WINO_TILE + half * 256


def store_cycles(addrs):
    """ds_write_b64: lane groups of 16 contiguous lanes, two dwords per lane, bank = (a/4) % 32"""
    tot = 0
    for g in WRITE_GROUPS:
        banks = {}
        for lane in g:
            for b in range(2):
                banks.setdefault(((addrs[lane] // 4) + b) % 32, set()).add(addrs[lane] + 4 * b)
        tot += max(len(v) for v in banks.values())
    return tot


def wino_read_cycles(mapping):
    """{(fragment index, p, kk, xi, half): LDS cycles of the wave's ds_read_b128}"""
    out = {}
    for fi, frag in enumerate(wino_fragments(mapping)):
        for p in range(2):
            for kk in range(4):
                for xi in range(4):
                    for half in range(2):
                        out[(fi, p, kk, xi, half)] = cycles([wino_read_addr(mapping, l, p, frag, kk, xi, half) for l in range(64)])
    return out


def wino_store_cycles(mapping):
    """{(wave, p, sel, xi, half): LDS cycles of the wave's 8-byte store}"""
    out = {}
    for wave in range(8):
        for p in range(2):
            for sel in range(2):
                for xi in range(4):
                    for half in range(2):
                        out[(wave, p, sel, xi, half)] = store_cycles(
                            [wino_store_addr(mapping, l, wave, p, sel, xi, half) for l in range(64)])
    return out


def wino_image_errors(mapping):
    """Every on-board read must return the eight channels 32*kk + 8*g4 .. + 7 of tile (p, row, j), tap xi, as the epilogue
    stored them; -> list of mismatches (empty = the store and the read addresses agree)."""
    mem = {}
    for wave in range(8):
        for p in range(2):
            for sel in range(2):
                for xi in range(4):
                    for half in range(2):
                        for lane in range(64):
                            g4, c = lane >> 4, lane & 15
                            y, j = wino_row(mapping, c >> 2, sel), c & 3
                            a = wino_store_addr(mapping, lane, wave, p, sel, xi, half)
                            for r in range(4):
                                assert a + 2 * r not in mem, "two stores to one address"
                                mem[a + 2 * r] = (p, y, j, xi, half, 16 * wave + 4 * g4 + r)
    bad = []
    for fi, frag in enumerate(wino_fragments(mapping)):
        for p in range(2):
            for kk in range(4):
                for xi in range(4):
                    for half in range(2):
                        for lane in range(64):
                            g4, c = lane >> 4, lane & 15
                            y, j = frag(c >> 2), c & 3
                            a = wino_read_addr(mapping, lane, p, frag, kk, xi, half)
                            if not 0 <= y < 8:
                                if not (ZERO <= a and a + 16 <= ZERO + 4 * WINO_TILE):
                                    bad.append(("zero block", fi, p, kk, xi, half, lane, a))
                                continue
                            for e in range(8):
                                if mem.get(a + 2 * e) != (p, y, j, xi, half, 32 * kk + 8 * g4 + e):
                                    bad.append((fi, p, kk, xi, half, lane, e, mem.get(a + 2 * e)))
    return bad


if __name__ == "__main__":
    for name, fn, nt, nk, key in (("16x16x32, key16 (shipped)", addr16, 16, 4, key16),
                                  ("16x16x32, key32-style (x | p<<3)", addr16, 16, 4, lambda xs, p: (xs & 7) | ((p & 1) << 3)),
                                  ("32x32x16, key32 (shipped)", addr32, 8, 8, key32)):
        c = n = 0
        for tap in range(9):
            for t in range(nt):
                for kk in range(nk):
                    c += cycles([fn(l, t, tap, kk, key) for l in range(64)])
                    n += 1
        print("%-28s %.2f LDS cycles per ds_read_b128" % (name, c / n))
    for mapping in WINO_MAPPINGS:
        rd, st = wino_read_cycles(mapping), wino_store_cycles(mapping)
        nfrag = len(wino_fragments(mapping))
        print("k_trunk_w, %-7s %d fragments per (position, k-step, xi): %.2f (max %d) LDS cycles per ds_read_b128; "
              "%.2f (max %d) per 8-byte epilogue store; image %s"
              % (mapping + ":", nfrag, sum(rd.values()) / len(rd), max(rd.values()), sum(st.values()) / len(st),
                 max(st.values()), "consistent" if not wino_image_errors(mapping) else "INCONSISTENT"))
