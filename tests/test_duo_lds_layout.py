"""CPU restatement of the dense duo loop kernel's LDS layout (csrc/wrnn_duo.hip `duo_lds`, csrc/wrnn_tiles.h `put_partial` /
`get_partial`): the cross-wave partial-tile exchange and the carve it lives in.

The partial tiles keep the accumulators' own fragment order: a layout in which the four waves' partials of one (tile, unit, segment)
are adjacent -- one 16-byte read per gate instead of four 4-byte ones -- would have to be WRITTEN word by word (a wave's 16-byte
accumulator word holds four units of ONE wave), four stores per tile instead of one; the exchange was left as it is, and this file pins
what the kernel relies on: every word a wave puts is read by exactly the thread that owns that (unit, segment), the four partials in wave
order 0..3, nothing is read that was not put, and the two ping-pong sets stay inside their region for every depth.
"""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = open(os.path.join(ROOT, 'wavernn_amd', 'csrc', 'wrnn_duo.hip')).read()
TILES = open(os.path.join(ROOT, 'wavernn_amd', 'csrc', 'wrnn_tiles.h')).read()

NW, SEG, LDC, LMAXG, DNWGC, DLOGS, NSLOT = 4, 16, 520, 8, 128, 36, 3
SET = NW * NSLOT * 256                      # floats of one ping-pong set
LDS_PER_CU = 160 * 1024


def put_partial(w, s, lane, r):
    """word index (inside a set) of element r of wave w's accumulator word of tile s: row 4 (lane >> 4) + r, segment lane & 15"""
    return (w * NSLOT + s) * 256 + lane * 4 + r


def get_partial(base, ri, j):
    """word indices, in summation order, that the owner of (tile base, row ri, segment j) adds up"""
    o = (base + (ri >> 4)) * 256 + (((ri & 15) >> 2) * 16 + j) * 4 + (ri & 3)
    return [o + w * NSLOT * 256 for w in range(NW)]


def duo_lds(G):
    regions, o = {}, 0

    def take(name, n):
        nonlocal o
        regions[name] = (o, o + n)
        o += n
    take('h', G * 256)
    take('seg', G * 48)
    take('xs', G * 16)
    take('part', 2 * SET)
    take('log', SEG * DLOGS)
    take('misc', 2 * LMAXG + 2 * DNWGC)
    take('prof', 2 * 16)
    o = (o + 3) & ~3
    take('f3', SEG * LDC)
    return regions, o


def test_source_still_says_what_is_restated_here():
    assert 'part + (w * NSLOT + s) * 256 + lane * 4' in TILES
    assert 'const int o = (base + (ri >> 4)) * 256 + (((ri & 15) >> 2) * 16 + j) * 4 + (ri & 3);' in TILES
    assert 's += part[w * NSLOT * 256 + o]' in TILES and 'for (int w = 1; w < NW; ++w)' in TILES
    assert 'constexpr int DPART = 2 * NW * 3 * 256;' in SRC
    assert '#define DPARTOF(q) (PART + (q) * (NW * 3 * 256))' in SRC
    carve = re.search(r'inline DuoLds duo_lds\(int G\)\s*\{(.*?)\n\}', SRC, re.S).group(1)
    sizes = re.findall(r'l\.off_(\w+) = o;\s*o \+= ([^;]+);', carve)
    assert sizes == [('h', 'G * 256'), ('seg', 'G * 48'), ('xs', 'G * 16'), ('part', 'DPART'), ('log', 'SEG * DLOGS'),
                     ('misc', '2 * LMAXG + 2 * DNWGC'), ('prof', '2 * 16'), ('f3', 'SEG * LDC')]
    assert 'const int pu = 4 * w + (tid & 3), pj = (tid >> 2) & 15;' in SRC


def test_every_word_put_is_read_by_its_owner_in_wave_order():
    for s in range(NSLOT):
        readers = {}                                  # word -> (thread, position in its sum)
        for tid in range(NW * 64):
            w_r = tid >> 6
            pu, pj = 4 * w_r + (tid & 3), (tid >> 2) & 15
            words = get_partial(s, pu, pj)
            for k, o in enumerate(words):
                assert o not in readers
                readers[o] = (tid, k, pu, pj)
        put = {}
        for w in range(NW):
            for lane in range(64):
                for r in range(4):
                    o = put_partial(w, s, lane, r)
                    assert o not in put and 0 <= o < SET
                    put[o] = (w, 4 * (lane >> 4) + r, lane & 15)
        assert set(put) == set(readers)               # nothing is read that was not put, nothing put is left unread
        for o, (w, row, seg) in put.items():
            tid, k, pu, pj = readers[o]
            assert (pu, pj) == (row, seg)             # ... by the thread that owns that (unit, segment)
            assert k == w                             # ... as the w-th term of its sum: wave order 0, 1, 2, 3
        # a reader wave's 64 lanes read 64 consecutive words per term (conflict-free), a writer wave 256 consecutive ones
        for w_r in range(NW):
            for k in range(NW):
                ws = sorted(get_partial(s, 4 * w_r + (l & 3), (l >> 2) & 15)[k] for l in range(64))
                assert ws == list(range(ws[0], ws[0] + 64))


def test_ping_pong_sets_stay_inside_their_region_for_every_depth():
    for G in range(1, LMAXG + 1):
        regions, total = duo_lds(G)
        spans = sorted(regions.values())
        for (a0, a1), (b0, b1) in zip(spans, spans[1:]):
            assert a0 < a1 <= b0                      # the regions are disjoint
        p0, p1 = regions['part']
        sets = [(p0 + q * SET, p0 + (q + 1) * SET) for q in range(2)]
        assert sets[0][1] == sets[1][0] and sets[1][1] == p1
        for q in range(2):
            words = {sets[q][0] + put_partial(w, s, lane, r) for w in range(NW) for s in range(NSLOT) for lane in range(64) for r in range(4)}
            assert min(words) == sets[q][0] and max(words) == sets[q][1] - 1
        assert regions['f3'][0] % 4 == 0 and p0 % 4 == 0          # 16-byte words
        assert 2 * total * 4 <= LDS_PER_CU            # two workgroups per CU
