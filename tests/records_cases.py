"""The stage-1 record kernels' cases, restated in Python: the first-token rule of nsnp_mpileup_line_names, the numpy model of
nsnp_pileup_window_records (per-site names included) and the seeded builders of the texts that bring pileup_records.hip and
pipeline.contig_to_bin to the shapes real chunks have.  Test infrastructure shared by the CPU tests that assert every builder's
preconditions (tests/test_pileup_bins_host.py) and the GPU tests whose expectations rest on them (tests/test_gpu_pileup_bins.py)."""
import functools

import numpy as np

NM_TILE = 4096                 # bytes of text per block of k_names_count / k_names_emit
SCAN_THREADS = 1024            # threads of k_names_scan / k_alt_scan: each owns ceil(n / 1024) entries
COPY_SWEEP = 1024 * 256 * 16   # bytes k_alt_copy's largest grid moves before its grid-stride loop runs: 4,194,304
NAME_ENTRY = 44                # 40 name bytes, then the length as int32
NAME_MAX = 37                  # 37 + 1 + 11 + 1 + 33 = 83
NO_ROOM = 0x7fffffff           # a line_idx entry the name table had no room for
FIRST_ROWS = 1024              # rows of a record slot created for a small chunk


def scan_per(n):
    """entries per thread of the one-block scans"""
    return -(-n // SCAN_THREADS)


def n_tiles(n_bytes):
    return -(-n_bytes // NM_TILE)


# ---- the first-token rule ------------------------------------------------------------------------------------------------------------
def text_lines(text):
    """the tokeniser's lines: a line starts at offset 0 and behind every newline (no empty lines in these texts)"""
    lines = bytes(text).split(b"\n")
    return lines[:-1] if lines and not lines[-1] else lines


def first_token(line):
    """split_line: leading tabs are skipped, the token ends at the next tab (or at the end of the line)"""
    return line.lstrip(b"\t").split(b"\t")[0]


def line_names_rule(text, name):
    """-> (the first token of every line, the indices of the lines whose token is not `name`)"""
    toks = [first_token(l) for l in text_lines(text)]
    return toks, [i for i, t in enumerate(toks) if t != name]


def name_entry(tok):
    """the 44 bytes nsnp_mpileup_line_names keeps of a token: its first 40 bytes, zero-padded, and its whole length"""
    e = np.zeros(NAME_ENTRY, np.uint8)
    e[:min(len(tok), 40)] = np.frombuffer(tok[:40], np.uint8)
    e[40:44] = np.frombuffer(np.int32(len(tok)).tobytes(), np.uint8)
    return e


# ---- the numpy model of nsnp_pileup_window_records ------------------------------------------------------------------------------------
def np_records(counts, centers, pos, seq, name, elem, line_idx=None, names=None):
    """-> (position_matrix [N,33,18], position [N,83], refused): a site's name is the contig's unless line_idx[centre + 16] names an entry
    of `names` ([E,44] uint8: 40 name bytes, then the int32 length); a length outside 1..37 is clamped and an entry of NO_ROOM falls back to
    the contig's name, both with `refused` set (meta[2] of the call)"""
    n, m = centers.size, counts.shape[0]
    c = np.clip(centers, 16, m - 17)
    x = counts[c[:, None] + np.arange(-16, 17)[None, :]] if n else np.empty((0, 33, 18), np.int32)
    out = np.zeros((n, 83), np.uint8)
    up = seq.copy()
    low = (up >= ord("a")) & (up <= ord("z"))
    up[low] -= 32
    refused = False
    for i in range(n):
        p = int(pos[c[i]])
        q = min(max(p, 0), 10 ** 11 - 1)
        idx = np.clip(np.arange(q - 17, q + 16), 0, seq.size - 1)
        nm = name
        if line_idx is not None:
            e = int(line_idx[c[i] + 16])
            if e == NO_ROOM:
                refused = True
            elif e >= 0:
                nlen = int(names[e, 40:44].view(np.int32)[0])
                if nlen < 1 or nlen > NAME_MAX:
                    refused = True
                    nlen = 1 if nlen < 1 else NAME_MAX
                nm = names[e, :nlen].tobytes()
        s = nm + b":" + str(q).encode() + b":" + up[idx].tobytes()
        out[i, :len(s)] = np.frombuffer(s, np.uint8)
    return x.astype(np.int16 if elem == 2 else np.int32), out, refused


SITE_NAME_LENGTHS = (1, 2, 36, 37)
# which name consecutive sites carry (-1: the contig's): every entry beside the contig's name on either side, then entries of different
# lengths side by side
SITE_NAME_PATTERN = (-1, 0, -1, 1, -1, 2, -1, 3, -1, 3, 0, 2, 1, 3, 1, 0)


def site_names_case(n, m, seed=0):
    """n sites on CONSECUTIVE centres 16 .. 16 + n - 1 of m columns -> (centres [n], line_idx [m] int32, names [8,44]): site j's emitting
    line (centre + 16) carries SITE_NAME_PATTERN[j % 16]; two entries per length of SITE_NAME_LENGTHS, the 40 name bytes behind a name
    filled with 0xAA (only the length says where a name ends)"""
    assert 16 + n - 1 <= m - 17
    rng = np.random.default_rng(1000 + seed)
    names = np.full((8, NAME_ENTRY), 0xAA, np.uint8)
    for e in range(8):
        nlen = SITE_NAME_LENGTHS[e % 4]
        names[e, :nlen] = rng.choice(np.frombuffer(b"abcdefghijklmnopqrstuvwxyz_0123456789", np.uint8), nlen)
        names[e, 40:44] = np.frombuffer(np.int32(nlen).tobytes(), np.uint8)
    centers = np.arange(16, 16 + n, dtype=np.int64)
    line_idx = np.full(m, -1, np.int32)
    for j in range(n):
        k = SITE_NAME_PATTERN[j % 16]
        line_idx[centers[j] + 16] = -1 if k < 0 else k + 4 * ((j // 16) % 2)
    return centers, line_idx, names


# ---- texts for nsnp_mpileup_line_names above 1,024 tiles ------------------------------------------------------------------------------
LN_NAME = b"chrR"
LN_TOKENS = (b"X", b"chr", b"chrr", b"chrRx", b"some_other_name", b"c" * 37, b"e" * 40, b"d" * 45)     # none equals LN_NAME
LN_LONG = 9000                 # a line longer than two tiles: a whole tile inside it holds no newline


def _fill(rng, cur, target):
    """line lengths (newline included, 30 .. 70 bytes) that lead from offset cur exactly to offset target (target - cur > 70)"""
    out = []
    while target - cur > 140:
        l = int(rng.integers(30, 71))
        out.append(l); cur += l
    gap = target - cur
    out += [gap // 2, gap - gap // 2]
    return out


def names_anchors(tiles):
    """{offset: kind} of the lines a text of `tiles` tiles places on purpose (tile t starts at 4096 t; per = entries per scan thread):
    a token or a run of four leading tabs that starts two bytes in front of a tile edge and ends behind it, a line that starts on the first
    byte of a tile, and two long lines - one covers the first tiles scan thread 300 owns, one the last tile thread 41 owns"""
    per = scan_per(tiles)
    T = NM_TILE
    return {
        (per * 15) * T - 2: "tok_same", (per * 7) * T - 2: "tok_other", (per * 9 + per - 1) * T - 2: "tabs_same", (per * 11 + 1) * T - 2: "tabs_other",
        3 * T: "edge_other", (per * 13) * T: "edge_other", (tiles - 2) * T: "edge_other", (tiles - 3) * T - 2: "tok_other",
        (per * 300) * T - 100: "long", (per * 41 + per - 1) * T - 50: "long",
    }


@functools.lru_cache(maxsize=None)
def _names_layout(tiles):
    """the lines of a text up to 300 bytes in front of its last tile: (lengths, kinds)"""
    rng = np.random.default_rng(tiles)
    lens, kinds, cur = [], [], 0
    stop = (tiles - 1) * NM_TILE - 300
    for off, kind in sorted(names_anchors(tiles).items()) + [(stop, "end")]:
        f = _fill(rng, cur, off)
        lens += f; kinds += ["plain"] * len(f); cur = off
        if kind != "end":
            l = LN_LONG if kind == "long" else int(rng.integers(50, 71))
            lens.append(l); kinds.append(kind); cur += l
    return lens, kinds


def names_marked_tiles(tiles):
    """the tiles whose first and last line start carry another token: tile 0, the last tiles (those the scan's threads without work would
    own if their range were clamped to the last entry instead of to none), the first and last tile of several scan threads"""
    per = scan_per(tiles)
    last_owner = (tiles - 1) // per
    want = {0, 1, tiles - 1, tiles - 2, tiles - 3}
    for k in (0, 1, 2, 63, 64, 255, 256, 300, 301, last_owner - 1, last_owner):
        want |= {k * per, k * per + per - 1}
    return sorted(t for t in want if 0 <= t < tiles)


def names_text(tiles, rest, newline):
    """a text of exactly `tiles` tiles for nsnp_mpileup_line_names -> (text, name).  rest: the bytes of the last tile (1: one more than a
    multiple of 4,096; 4095: one less than one; 4096: a multiple); newline: whether the last line ends in one.  Lines of 30 to 70 bytes
    and two of LN_LONG; another token than the name on the lines of names_anchors, on the first and the last line start of every tile of
    names_marked_tiles, beside the long lines and on one seeded line in 150"""
    lens, kinds = _names_layout(tiles)
    lens, kinds = list(lens), list(kinds)
    total = (tiles - 1) * NM_TILE + rest
    rng = np.random.default_rng(tiles * 8 + rest % 7 + newline)
    f = _fill(rng, sum(lens), total)
    lens += f; kinds += ["plain"] * len(f)
    starts = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)
    tile_of = starts // NM_TILE
    other = rng.random(len(lens)) < 1 / 150
    for t in names_marked_tiles(tiles):
        here = np.flatnonzero(tile_of == t)
        if here.size:
            other[here[0]] = other[here[-1]] = True
    for i, k in enumerate(kinds):
        if k == "long":
            other[i - 1] = other[i + 1] = True
            other[i] = False
        elif k != "plain":
            other[i] = k.endswith("_other")
    other[-1] = True                                                   # (the last line, with or without its newline)
    out = []
    for i, (l, k) in enumerate(zip(lens, kinds)):
        body = l - 1 if (newline or i + 1 < len(lens)) else l          # (the last line without a newline is one byte longer instead)
        lead = b"\t" * 4 if k.startswith("tabs") else b""
        tok = LN_NAME
        if other[i]:
            fits = [t for t in LN_TOKENS if len(lead) + len(t) + 20 <= body and (k != "tok_other" or len(t) > 2)]     # (over the edge)
            tok = fits[int(rng.integers(0, len(fits)))] if i % 5 else fits[-1]      # (every fifth: the longest that fits)
        head = lead + tok + b"\t%d\tN\t3\t" % (i + 1)
        fill = body - len(head) - 4
        assert fill >= 1, (i, l, k, tok)
        out.append(head + b"A" * fill + b"\tIII")
    text = b"\n".join(out) + (b"\n" if newline else b"")
    assert len(text) == total
    return text, LN_NAME


# ---- the alt_info fixture -----------------------------------------------------------------------------------------------------------
def alt_text():
    """-> (contig, seq, mpileup text, {kind: 1-based position}): consecutive positions 1..L, the special columns far enough apart and from
    the ends to be the centre of 33 consecutive positions, 6,000 columns of random printable bytes behind them"""
    rng = np.random.default_rng(41)
    specials = {}
    seq = rng.choice(np.frombuffer(b"ACGT", np.uint8), 40 + 40 * 12 + 6000 + 17).astype(np.uint8)
    seq[rng.random(seq.size) < 0.1] |= 0x20                              # lower-case reference bases among them

    def other(r, k=0):
        return [b for b in b"CGTA" if b != (r & 0xDF)][k:k + 1]

    def plain(p):
        r = bytes([seq[p - 1] & 0xDF])
        return r * 8 + r.lower() * 4

    def special(kind, make):
        p = 40 + 40 * len(specials)
        specials[kind] = p
        return p, make(bytes([seq[p - 1] & 0xDF]), bytes(other(seq[p - 1])), p)

    let = b"ACGTNRYK"                                                    # (distinct after upper-casing too: 500 keys)
    distinct = [bytes(let[(k // 8 ** j) % 8] for j in range(3)) for k in range(500)]
    makers = [
        ("500 distinct insertions", lambda r, o, p: o * 10 + b"".join(b"+3" + a for a in distinct)),
        ("same allele in both cases", lambda r, o, p: r * 10 + b"+2ac" * 3 + b"+2AC" * 4 + b"+2Ac" + b"-2gt" * 2 + b"-2GT"),
        ("+0 and -0", lambda r, o, p: o * 7 + b"+0" + r * 3 + b"-0" + b"+" + b"-"),
        ("cut insertion beside the complete one", lambda r, o, p: o * 9 + b"+2AC+2AC+2ac+3AC"),
        ("deletions of 60 and 61", lambda r, o, p: r * 10 + (b"-60" + b"N" * 60) * 2 + (b"-61" + b"N" * 61) * 3),
        ("longer than 5000 bytes", lambda r, o, p: o * 10 + b"+3ACG" * 1200 + r * 20),
        ("counts of 1 to 4 digits", lambda r, o, p: o * 10 + b"+1A" + b"+1C" * 12 + b"+1G" * 123 + b"+2TT" * 1234),
        ("indel only", lambda r, o, p: r * 6 + r.lower() * 4 + b"+2GT" * 5),
        ("mismatches of three bases in both cases", lambda r, o, p: bytes(other(r[0], 0) * 3 + other(r[0], 1) * 2 + other(r[0], 2)) + bytes(other(r[0], 0)).lower() * 4 + r * 2),
    ]
    by_pos = {}
    for kind, make in makers:
        p, c = special(kind, make)
        by_pos[p] = c
    n_front = 40 + 40 * 12
    L = seq.size
    # the last column a window can be centred on: its deletions reach past the end of the contig
    p_end = L - 16
    specials["deletion past the end"] = p_end
    o = bytes(other(seq[p_end - 1]))
    by_pos[p_end] = o * 10 + b"-3ACG" * 2 + b"-20" + b"A" * 20 + b"-40" + b"C" * 40 + b"+2GG" * 3
    rnd = iter(bytes(rng.integers(33, 127, int(rng.integers(1, 300)), dtype=np.uint8)) for _ in range(6000))
    lines = []
    for p in range(1, L + 1):
        c = by_pos.get(p) or (plain(p) if p <= n_front or p > n_front + 6000 else next(rnd))
        lines.append(b"ctgA\t%d\tN\t%d\t%s\t%s\n" % (p, len(c), c, b"I"))
    return "ctgA", seq, b"".join(lines), specials


def oracle_pd(tmp_dir, text, seq, tag="t"):
    """the oracle's .pd of a text (bytes) and its site count"""
    from oracle import oracle
    src, dst = tmp_dir / f"{tag}.mpileup", tmp_dir / f"{tag}.pd"
    src.write_bytes(text)
    n = oracle.mpileup_to_pd(str(src), np.asarray(seq, np.uint8).tobytes(), str(dst))
    pd = dst.read_bytes()
    assert pd.count(b"\n") == n
    return pd, n


def pd_fields(pd):
    """-> [(name, position, alt_info)] of a .pd's lines"""
    out = []
    for line in pd.split(b"\n"):
        if line:
            _, position, alt = line.split(b"\t", 2)
            name, p, _ = position.rsplit(b":", 2)
            out.append((name, int(p), alt))
    return out


def alt_case_data(tmp_dir):
    """the alt_info text, its columns and the oracle's .pd"""
    from nanosnp_amd import host
    from oracle import oracle
    contig, seq, text, specials = alt_text()
    pd, n = oracle_pd(tmp_dir, text, seq, "a")
    want = {p: alt for _, p, alt in pd_fields(pd)}
    assert len(want) == n
    pos, off, bases = host.mpileup_parse(text)
    ref = seq[pos - 1]
    _, depth, _ = oracle.encode_columns(bases, off, ref)
    return dict(contig=contig, seq=seq, text=text, specials=specials, want=want, pos=pos, off=off, bases=bases, ref=ref, depth=depth, pd=pd)


ALT_SCAN_N = (1, 1023, 1024, 1025, 2048, 2049)                           # per 1, 1, 1, 2, 2, 3


def alt_scan_centers(want, n):
    """n centres (column indices: position - 1) drawn with repeats, in a seeded order, from the sites the oracle selected"""
    sites = np.array(sorted(want), np.int64)
    return sites[np.random.default_rng(7000 + n).integers(0, sites.size, n)] - 1


def alt_sweep_centers(want, specials, repeats=1100):
    """the "500 distinct insertions" column `repeats` times, a short-text site between every two of them, then short sites until the
    total is no multiple of 16 -> (centres, total bytes)"""
    big = specials["500 distinct insertions"]
    short = [p for p in sorted(want) if len(want[p]) < 40 and p != big]
    rng = np.random.default_rng(7)
    ps = []
    for _ in range(repeats):
        ps += [big, short[int(rng.integers(0, len(short)))]]
    total = sum(len(want[p]) for p in ps)
    k = 0
    while total % 16 == 0 or total <= COPY_SWEEP + 16:
        ps.append(short[k]); total += len(want[short[k]]); k += 1
    return np.array(ps, np.int64) - 1, total


# ---- texts for contig_to_bin ----------------------------------------------------------------------------------------------------------
OTHER_NAMES = (b"x", b"ab", b"some_other_name", b"n" * 36, b"m" * 37)


def rename_lines(text, n_other, seed):
    """column 0 of n_other seeded lines of a text replaced by one of OTHER_NAMES -> (text, the line indices)"""
    lines = text_lines(text)
    rng = np.random.default_rng(seed)
    which = np.sort(rng.choice(len(lines), n_other, replace=False))
    for j, i in enumerate(which):
        lines[i] = OTHER_NAMES[j % len(OTHER_NAMES)] + lines[i][lines[i].index(b"\t"):]
    return b"\n".join(lines) + b"\n", which


def synth_text(seed, n_cols, contig):
    """host.synth_columns at coverage 30, 5 % heterozygous -> (text, seq)"""
    from nanosnp_amd import host
    cols = host.synth_columns(seed, n_cols, coverage=30, het_rate=0.05)
    return bytes(cols.mpileup_text_native(contig)), cols.ref.copy()


def chunk_lines(text, chunk_bytes):
    """the pipeline's chunks of a text -> [(first own line, end of own lines, first line with halo, end with halo)] in line indices"""
    from nanosnp_amd.pipeline import halo_range, ramp_cuts
    cuts = ramp_cuts(text, 0, len(text), chunk_bytes)
    starts = np.concatenate([[0], np.flatnonzero(np.frombuffer(text, np.uint8) == 10) + 1])
    line_at = lambda o: int(np.searchsorted(starts, o))
    out = []
    for a, b in zip(cuts[:-1], cuts[1:]):
        lo, hi, _, _ = halo_range(text, a, b)
        out.append((line_at(a), line_at(b), line_at(lo), line_at(hi)))
    return out, [b - a for a, b in zip(cuts[:-1], cuts[1:])]


DEEP_READS = 33_000
DEEP_CHUNK = 16384             # chunk_bytes at which deep_text() is more than one chunk
GROWN_COLS, GROWN_OTHER, GROWN_CHUNK = 185_000, 3_000, 5_000_000     # a text of three chunks and more, two of them above 4 MiB


def _plain_line(name, p, seq):
    r = bytes([seq[p - 1] & 0xDF])
    return b"%s\t%d\tN\t12\t%s\tI\n" % (name, p, r * 8 + r.lower() * 4)


def _deep_line(name, p, seq):
    r = seq[p - 1] & 0xDF
    o = bytes([b for b in b"CGTA" if b != r][:1])
    return b"%s\t%d\tN\t%d\t%s\tI\n" % (name, p, DEEP_READS + 10, o * DEEP_READS + bytes([r]) * 10)


def deep_text(n_lines=1500, deep_at=300, contig=b"deep"):
    """consecutive positions 1..n_lines of reference reads only, but column deep_at: 33,000 mismatching reads and 10 reference reads
    -> (contig, seq, text)"""
    seq = np.random.default_rng(51).choice(np.frombuffer(b"ACGT", np.uint8), n_lines).astype(np.uint8)
    lines = [_deep_line(contig, p, seq) if p == deep_at else _plain_line(contig, p, seq) for p in range(1, n_lines + 1)]
    return contig.decode(), seq, b"".join(lines)


def big_insertions(n=120):
    let = b"ACGTNRYK"
    return b"".join(b"+3" + bytes(let[(k // 8 ** j) % 8] for j in range(3)) for k in range(n))


def outgrown_blob_text(contig=b"big"):
    """300 lines, positions 50..249 with 120 distinct insertions each: 200 neighbouring sites whose alt_info (about 1 KB a site) does not
    fit the blob budgeted for a first slot (64 bytes a site + 64 KB) -> (contig, seq, text)"""
    seq = np.random.default_rng(43).choice(np.frombuffer(b"ACGT", np.uint8), 300).astype(np.uint8)
    ins = big_insertions()
    lines = [b"%s\t%d\tN\t10\t%s\tI\n" % (contig, p, bytes([seq[p - 1]]) * 10 + (ins if 50 <= p < 250 else b"")) for p in range(1, 301)]
    return contig.decode(), seq, b"".join(lines)


def three_causes_text(contig=b"tri"):
    """one text with three reasons to start a contig over: 200 neighbouring sites of 120 distinct insertions (positions 50..249: their
    alt_info outgrows a first slot's blob), the deep column at 1,000 (a count outside int16) and another name on two lines in three of
    positions 40..1,799 (more than the name table's 1,024 entries) -> (contig, seq, text, the indices of the renamed lines)"""
    n_lines = 2000
    seq = np.random.default_rng(52).choice(np.frombuffer(b"ACGT", np.uint8), n_lines).astype(np.uint8)
    ins = big_insertions()
    lines, renamed = [], []
    for p in range(1, n_lines + 1):
        name = contig
        if 40 <= p < 1800 and p % 3:
            name = OTHER_NAMES[p % len(OTHER_NAMES)]
            renamed.append(p - 1)
        if 50 <= p < 250:
            lines.append(b"%s\t%d\tN\t10\t%s\tI\n" % (name, p, bytes([seq[p - 1]]) * 10 + ins))
        elif p == 1000:
            lines.append(_deep_line(name, p, seq))
        else:
            lines.append(_plain_line(name, p, seq))
    return contig.decode(), seq, b"".join(lines), renamed


SLOT_CHUNK = 512 << 10


def slot_growth_text(contig=b"grow"):
    """a text whose first three chunks at chunk_bytes = SLOT_CHUNK select a few sites each and whose fourth selects more than a first
    slot's rows: 50,000 columns of reference reads with one mismatch column in every 4,000, then 3,600 dense columns of random printable
    bytes -> (contig, seq, text)"""
    rng = np.random.default_rng(53)
    n_plain, n_dense = 50_000, 3_600
    n_lines = n_plain + n_dense + 40
    seq = rng.choice(np.frombuffer(b"ACGT", np.uint8), n_lines).astype(np.uint8)
    lines = []
    for p in range(1, n_lines + 1):
        if n_plain < p <= n_plain + n_dense:
            c = bytes(rng.integers(33, 127, int(rng.integers(1, 300)), dtype=np.uint8))
            lines.append(b"%s\t%d\tN\t%d\t%s\tI\n" % (contig, p, len(c), c))
        elif p <= n_plain and p % 4000 == 2000:
            o = bytes([b for b in b"CGTA" if b != seq[p - 1]][:1])
            lines.append(b"%s\t%d\tN\t12\t%s\tI\n" % (contig, p, o * 10 + bytes([seq[p - 1]]) * 2))
        else:
            lines.append(_plain_line(contig, p, seq))
    return contig.decode(), seq, b"".join(lines)


def sites_per_chunk(pd, text, chunk_bytes):
    """the oracle's sites of a text with positions 1..L on lines 0..L - 1, counted by the chunk that owns the centre's line"""
    chunks, _ = chunk_lines(text, chunk_bytes)
    lines = np.array([p - 1 for _, p, _ in pd_fields(pd)], np.int64)
    return [int(((lines >= a) & (lines < b)).sum()) for a, b, _, _ in chunks]
