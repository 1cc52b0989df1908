"""nsnp_mpileup_tokenise_contigs (mpileup_tokenise.hip) through its binding, on its own: pos / col_off / bases against the oracle's
restatement of the reference's reader (oracle.mpileup_tokenise), cid / ref / key / the run table against the Python restatement of the
splitter's name rule (tests/contig_rules.py, pinned to the reference's own output by tests/test_call_mpileup_host.py) - every output bit
for bit.  The kernels' tile is 8 KB: the small texts of 20-40 KB span several.  k_ctg_scan scans one entry per block of 256 lines in one
workgroup of 1,024 threads: up to 64 blocks (16,384 lines) stay inside one wave's scan, more go through the wave-to-wave step (sh_v / sh_l:
vb, lb, lt), more than 1,024 blocks (262,144 lines) through the round loop's carry_n / carry_l - the texts of short lines further down
are sized to reach each of them, and every one of them asserts that it does."""
import functools
import itertools

import numpy as np
import pytest

from oracle import oracle
from tests.contig_rules import FILLER, contig_rule

pytestmark = pytest.mark.gpu

NAMES = [b"chr1", b"chr10", b"chr1_KI270706v1_random", b"ctgA", b"ctgB"]
SEQS = [np.frombuffer(b"ACGTNacgt", np.uint8)[np.random.default_rng(40 + i).integers(0, 9, n)] for i, n in enumerate((900, 700, 650, 2000, 300))]


@pytest.fixture(scope="module")
def ctx():
    from nanosnp_amd import _lib
    c = _lib.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def table():
    from nanosnp_amd import _lib
    return _lib.ContigTable({n.decode(): s for n, s in zip(NAMES, SEQS)})


def L(name, p, sep=b"\t", qual=b"III"):
    return name + sep + b"%d\tN\t3\tAc.\t" % p + qual


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _expect(text, names=NAMES, seqs=SEQS):
    """(pos, col_off, bases) of the oracle's reader, (cid, ref, key, runs) of the name rule"""
    opos, ooff, obases = oracle.mpileup_tokenise(np.frombuffer(text, np.uint8))
    return (opos, ooff, obases) + contig_rule(text, names, seqs, opos)


def _check(ctx, table, text, shift=0, exp=None, names=NAMES, seqs=SEQS, stream=None, before=None):
    """every output == its expectation; shift: the text starts `shift` bytes into its device buffer; exp: _expect(text), where several
    runs share one text; before: called when the text is on the device, in front of the call on `stream`"""
    import torch
    t = np.frombuffer(text, np.uint8)
    buf = torch.full((t.size + shift + 64,), ord("\n"), dtype=torch.uint8, device="cuda")      # (bytes around the text must not be looked at)
    buf[shift:shift + t.size] = _dev(t)
    if before is not None:
        before()
    pos, off, bases, ref, cid, key, runs = ctx.mpileup_tokenise_contigs(buf[shift:shift + t.size], table, stream)
    opos, ooff, obases, ecid, eref, ekey, eruns = exp if exp is not None else _expect(text, names, seqs)
    assert np.array_equal(pos.cpu().numpy(), opos) and np.array_equal(off.cpu().numpy(), ooff) and np.array_equal(bases.cpu().numpy(), obases)
    assert cid.dtype == torch.int32 and np.array_equal(cid.cpu().numpy(), ecid)
    assert np.array_equal(ref.cpu().numpy(), eref)
    assert np.array_equal(key.cpu().numpy(), ekey)
    assert np.array_equal(runs.cpu().numpy(), eruns)
    return ecid, eruns


def _text(lines, tail=b"\n"):
    return b"\n".join(lines) + tail


def test_one_contig_equals_the_single_contig_tokeniser(ctx, table):
    text = _text([L(b"ctgA", p) for p in range(1, 1501)])
    assert len(text) > 3 * 8192
    cid, runs = _check(ctx, table, text)
    assert (cid == 3).all() and runs.tolist() == [[0, 3]]
    d = _dev(np.frombuffer(text, np.uint8))
    pos, off, bases, ref, _, _, _ = ctx.mpileup_tokenise_contigs(d, table)
    p1, o1, b1, r1 = ctx.mpileup_tokenise(d, _dev(SEQS[3]))
    for a, b in ((pos, p1), (off, o1), (bases, b1), (ref, r1)):
        assert np.array_equal(a.cpu().numpy(), b.cpu().numpy())


def test_three_contigs_and_runs_of_one_line(ctx, table):
    cid, runs = _check(ctx, table, _text([L(n, p) for n in (b"ctgB", b"chr1", b"ctgA") for p in range(1, 301)]))
    assert runs.tolist() == [[0, 4], [300, 0], [600, 3]]
    cyc = [NAMES[i % 5] for i in range(600)]
    cid, runs = _check(ctx, table, _text([L(n, 1 + i // 5) for i, n in enumerate(cyc)]))
    assert len(runs) == 600 and runs[:, 0].tolist() == list(range(600))


def test_a_b_a_and_prefix_names_in_every_order(ctx, table):
    cid, runs = _check(ctx, table, _text([L(n, p) for n in (b"ctgA", b"ctgB", b"ctgA") for p in range(1, 251)]))
    assert runs.tolist() == [[0, 3], [250, 4], [500, 3]]
    for order in itertools.permutations(NAMES[:3]):
        cid, runs = _check(ctx, table, _text([L(n, p) for n in order for p in range(1, 121)]))
        assert runs[:, 1].tolist() == [NAMES.index(n) for n in order]


def test_unknown_names_and_text_ends(ctx, table):
    A, U = [L(b"ctgA", p) for p in range(1, 301)], [L(b"chrUn_x", p) for p in range(1, 201)]
    for lines in (U + A + A, A + U + [L(b"ctgB", 7)] * 200, A + A + U, U):
        cid, runs = _check(ctx, table, _text(lines))
        assert (cid == -1).sum() == 200
    assert _check(ctx, table, L(b"chr10", 5))[1].tolist() == [[0, 1]]                 # a single line, no newline
    assert _check(ctx, table, L(b"chr10", 5) + b"\n")[1].tolist() == [[0, 1]]
    _check(ctx, table, _text(A + [L(b"chr1", p) for p in range(1, 301)], tail=b""))
    _check(ctx, table, _text([l + b"\r" for l in A] + [L(b"chr1", p) + b"\r" for p in range(1, 301)], tail=b"\n"))
    _check(ctx, table, b"\r\n".join(A + [L(b"chr1", 3)]))


def test_the_name_ends_at_the_first_space_of_any_kind(ctx, table):
    lines = [L(b"ctgA", p) for p in range(1, 200)]
    lines += [b"\t" + L(b"ctgA", p) for p in range(1, 5)]                              # a leading tab: the empty name
    lines += [L(b"ctgA", p, sep=b" \t") for p in range(5, 9)]                          # a space in front of the tab
    lines += [L(b"ctgA junk", p) for p in range(9, 12)]                                # ... the same name still
    lines += [L(b"ctgA\vx", 12), L(b"ctgA\fy", 13), L(b"ctgA\rz", 14), L(b"ctgAB", 1), L(b"ctg", 1), L(b"ctgA", 15)]
    cid, runs = _check(ctx, table, _text(lines))
    assert cid[199:203].tolist() == [-1] * 4 and cid[203:213].tolist() == [3] * 10 and cid[213:].tolist() == [-1, -1, 3]
    assert runs[:, 0].tolist() == [0, 199, 203, 213, 214, 215]


@pytest.mark.parametrize("shift", [0, 1, 7, 16])
def test_a_name_that_straddles_a_tile_boundary(ctx, table, shift):
    """the run start's name begins 3 bytes in front of a multiple of 8192 (of the second and of the third tile)"""
    lines, size = [], 0
    for boundary, name, nxt in ((8192, b"ctgA", b"chr1_KI270706v1_random"), (16384, b"chr1_KI270706v1_random", b"chr10")):
        p = 1
        while boundary - 3 - size > 200:
            lines.append(L(name, p)); size += len(lines[-1]) + 1; p += 1
        lines.append(L(name, p, qual=b"I" * (boundary - 3 - size - len(L(name, p, qual=b"")) - 1))); size += len(lines[-1]) + 1
        assert size == boundary - 3
        lines.append(L(nxt, 1)); size += len(lines[-1]) + 1
    lines += [L(b"chr10", p) for p in range(2, 400)]
    cid, runs = _check(ctx, table, _text(lines), shift=shift)
    assert runs[:, 1].tolist() == [3, 2, 1]


def _into_guarded(ctx, table, text, cap_cols, cap_bytes, cap_runs):
    """the entry point on buffers LONGER than the capacities it is told (8 elements; bases 64 bytes; runs 8 rows), filled with guard values
    -> (meta, {name: whole buffer}, {name: (capacity, guard value)})"""
    import torch
    d = _dev(np.frombuffer(text, np.uint8))
    mk = lambda n, dt, v: torch.full((n,), v, dtype=dt, device="cuda")
    caps = dict(pos=(cap_cols, -7), off=(cap_cols + 1, -7), bases=(cap_bytes, 255), ref=(cap_cols, 255), cid=(cap_cols, -7), key=(cap_cols, -7),
                runs=(cap_runs, -7))
    b = dict(pos=mk(cap_cols + 8, torch.int64, -7), off=mk(cap_cols + 1 + 8, torch.int64, -7), bases=mk(cap_bytes + 64, torch.uint8, 255),
             ref=mk(cap_cols + 8, torch.uint8, 255), cid=mk(cap_cols + 8, torch.int32, -7), key=mk(cap_cols + 8, torch.int64, -7),
             runs=torch.full((cap_runs + 8, 2), -7, dtype=torch.int64, device="cuda"))
    meta = torch.zeros(4, dtype=torch.int64, pin_memory=True)
    ctx.mpileup_tokenise_contigs_into(d, table, *[b[n][:caps[n][0]] for n in ("pos", "off", "bases", "ref", "cid", "key", "runs")], meta)
    torch.cuda.synchronize()
    return meta.tolist(), b, caps


def _into(ctx, table, text, cap_runs=64):
    cap = len(text) // 10 + 2
    meta, b, _ = _into_guarded(ctx, table, text, cap, len(text), cap_runs)
    return meta, b["runs"], (b["pos"][:cap], b["ref"][:cap], b["cid"][:cap], b["key"][:cap])


def test_positions_outside_the_lines_own_contig(ctx, table):
    ok = [L(b"ctgB", p) for p in range(1, 301)] + [L(b"ctgA", p) for p in range(1, 301)]
    assert _into(ctx, table, _text(ok))[0] == [600, 1800, 0, 2]
    for bad in (0, 301):                                                               # ctgB holds 300 bases, ctgA 2000
        meta, _, _ = _into(ctx, table, _text(ok[:150] + [L(b"ctgB", bad)] + ok[150:]))
        assert meta[2] == ctx.TOK_EPOS and meta[0] == 601
        assert _into(ctx, table, _text(ok[:300] + [L(b"ctgA", bad)] + ok[300:]))[0][2] == (ctx.TOK_EPOS if bad == 0 else 0)
        meta, _, (pos, ref, cid, key) = _into(ctx, table, _text(ok[:300] + [L(b"chrUn_x", bad)] + ok[300:]))
        assert meta == [601, 1803, 0, 3] and cid[300].item() == -1 and ref[300].item() == ord("N") and key[300].item() == FILLER
    with pytest.raises(ValueError, match="outside the reference"):
        ctx.mpileup_tokenise_contigs(_dev(np.frombuffer(_text([L(b"ctgB", 301)]), np.uint8)), table)


def test_run_table_capacity_and_name_length(ctx, table):
    text = _text([L(NAMES[i % 5], 1 + i // 5) for i in range(40)])
    meta, runs, _ = _into(ctx, table, text, cap_runs=40)
    assert meta[2:] == [0, 40] and (runs[40:] == -7).all() and runs[:40, 0].tolist() == list(range(40))
    meta, runs, _ = _into(ctx, table, text, cap_runs=39)
    assert meta[2] == ctx.TOK_ERANGE and meta[3] == 40 and (runs[39:] == -7).all() and runs[:39, 0].tolist() == list(range(39))
    assert len(ctx.mpileup_tokenise_contigs(_dev(np.frombuffer(_text([L(NAMES[i % 5], 1) for i in range(3000)]), np.uint8)), table)[6]) == 3000
    # names of 255 bytes are read, longer ones refused - as the first name of a run and as its continuation
    n255 = b"x" * 255
    assert _into(ctx, table, _text([L(n255, 1)] * 3 + [L(n255[:-1] + b"y", 1)]))[0] == [4, 12, 0, 2]
    for lines in ([L(n255 + b"x", 1)], [L(b"ctgA", 1), L(n255 + b"x", 2)], [L(n255 + b"x", 1)] * 2):
        assert _into(ctx, table, _text(lines))[0][2] & ctx.TOK_ENAME


def test_a_table_beyond_the_keys_limits_is_refused(ctx, table):
    from nanosnp_amd import _lib
    for n, glen in ((len(table), 1 << 36), ((1 << 17) + 1, table.genome_len)):
        fake = type("Table", (), {"__len__": lambda self, n=n: n})()
        fake.__dict__.update(names_blob=table.names_blob, name_off=table.name_off, genome=table.genome, seq_off=table.seq_off, genome_len=glen)
        with pytest.raises(_lib.NanoSNPError, match="invalid argument"):
            _into(ctx, fake, _text([L(b"ctgA", 1)]))
    with pytest.raises(_lib.NanoSNPError):
        _lib.ContigTable({"a": np.zeros(4, np.uint8)} | {f"c{i}": np.zeros(1, np.uint8) for i in range(1 << 17)})


# ---- line counts that reach every level of k_ctg_scan --------------------------------------------------------------------------------
WAVE_LINES, ROUND_LINES = 256 * 64, 256 * 1024         # lines one wave of the scan covers / one round of its 1,024 threads
UNKNOWN = b"chrUn_x"


def S(name, i):
    """a short line (about 15 bytes); the position stays inside the shortest contig of the table (ctgB, 300 bases)"""
    return name + b"\t%d\tN\t1\tA\tI" % (1 + i % 250)


def _lines_of_runs(n_lines, starts):
    """n_lines short lines; starts: {line index: name} of the run starts (line 0 among them), every other line repeats the name in front"""
    assert 0 in starts and max(starts) < n_lines
    lines, name = [], None
    for i in range(n_lines):
        name = starts.get(i, name)
        lines.append(S(name, i))
    return lines


SPARSE_STARTS = (0, 255, 256, 257, WAVE_LINES - 1, WAVE_LINES, WAVE_LINES + 1, ROUND_LINES - 1, ROUND_LINES, ROUND_LINES + 1, 270_000 - 1)


@functools.lru_cache(maxsize=None)
def _sparse(travels):
    """270,000 lines = 1,055 blocks of 256: run starts on both sides of a block edge, of the scan's wave edge, of its round edge, and on the
    last line; names rotate through the table, two starts have unknown names.  No start lies between WAVE_LINES + 1 and ROUND_LINES - 1, so
    the contig of the start at WAVE_LINES + 1 reaches blocks 65 .. 127 inside wave 1's scan and blocks 128 .. 1023 through lb, and the
    contig of the start at ROUND_LINES - 1 is round 0's carry_l.
      travels = "unknown": those two starts are the unknown ones - contig -1 travels as a value, distinct from CG_NONE (a scan that took -1
                for "no start" would hand on the known contig in front of it);
      travels = "known":   the starts ON the wave edge and ON the round edge are the unknown ones, and known contigs travel (a lost lb
                would read -1).
    -> (text, _expect(text)), computed once per variant"""
    names = {s: NAMES[k % 5] for k, s in enumerate(SPARSE_STARTS)}
    if travels == "unknown":
        names[WAVE_LINES + 1], names[ROUND_LINES - 1] = UNKNOWN, b"chrUn_y"
    else:
        names[WAVE_LINES], names[ROUND_LINES] = UNKNOWN, b"chrUn_y"
    order = [names[s] for s in SPARSE_STARTS]
    assert all(a != b for a, b in zip(order, order[1:]))   # (every listed line does start a run)
    text = _text(_lines_of_runs(270_000, names))
    return text, _expect(text)


@pytest.mark.parametrize("shift", [0, 5])
@pytest.mark.parametrize("travels", ["unknown", "known"])
def test_sparse_run_starts_on_block_wave_and_round_edges(ctx, table, travels, shift):
    text, exp = _sparse(travels)
    opos, ecid, eruns = exp[0], exp[3], exp[6]
    # preconditions: the text reaches the round loop, and the run starts lie where the levels of the scan meet
    assert opos.size == 270_000 > ROUND_LINES > WAVE_LINES and (opos.size + 255) // 256 == 1055
    assert eruns[:, 0].tolist() == list(SPARSE_STARTS)
    assert {255, 256, 257, 16383, 16384, 16385, 262143, 262144, 262145, 269999} <= set(eruns[:, 0].tolist())
    unknown = (WAVE_LINES + 1, ROUND_LINES - 1) if travels == "unknown" else (WAVE_LINES, ROUND_LINES)
    assert [s for s, c in eruns.tolist() if c < 0] == list(unknown)
    inherited = ecid[WAVE_LINES + 1:ROUND_LINES - 1]                  # blocks 65 .. 1023 hold no start but the one on their last line
    assert (inherited == inherited[0]).all() and (inherited[0] == -1) == (travels == "unknown")
    assert ecid[ROUND_LINES + 1] >= 0 and (ecid[ROUND_LINES + 1:-1] == ecid[ROUND_LINES + 1]).all() and ecid[-1] != ecid[-2]
    _check(ctx, table, text, shift=shift, exp=exp)


@pytest.mark.parametrize("second", [b"ctgB", UNKNOWN], ids=["known", "unknown"])
def test_a_round_of_the_scan_without_any_run_start(ctx, table, second):
    """530,000 lines = 2,071 blocks = three rounds.  Starts at lines 0, 100 and 2 * 262,144 + 300 only: round 1 (blocks 1024 .. 2047) has
    lt == CG_NONE and must hand round 0's carry_l on - to its own blocks and to the blocks of round 2 in front of the last start.  The
    carried contig is a known one (a lost carry would read -1) and, in the second case, the unknown one (-1 must not read as "no start")"""
    last = 2 * ROUND_LINES + 300
    text = _text(_lines_of_runs(530_000, {0: b"ctgA", 100: second, last: b"chr10"}))
    exp = _expect(text)
    opos, ecid, eruns = exp[0], exp[3], exp[6]
    c = NAMES.index(second) if second in NAMES else -1
    assert opos.size == 530_000 > last > 2 * ROUND_LINES and (opos.size + 255) // 256 == 2071
    assert eruns.tolist() == [[0, 3], [100, c], [last, 1]]
    assert (ecid[100:last] == c).all() and (ecid[last:] == 1).all()   # round 1 and the head of round 2 inherit the start at line 100
    _check(ctx, table, text, exp=exp)


def test_every_line_a_run_start(ctx, table):
    """270,000 lines, each of another name than the line in front (the table's five and an unknown one in turn): 270,000 runs.  The run
    index of a line is carry_n + vb + ve + before: all large here; the binding's run capacity grows from 1,024 to the count in one step"""
    six = NAMES + [UNKNOWN]
    text = _text([S(six[i % 6], i) for i in range(270_000)])
    exp = _expect(text)
    eruns = exp[6]
    assert exp[0].size == 270_000 > ROUND_LINES
    assert len(eruns) == 270_000 and np.array_equal(eruns[:, 0], np.arange(270_000)) and eruns[:12, 1].tolist() == [0, 1, 2, 3, 4, -1] * 2
    _check(ctx, table, text, exp=exp)


def test_mixed_run_lengths_seeded(ctx, table):
    """run lengths drawn from three scales - 1 or 2 lines, up to 100, up to 10,000 - with unknown names among them, at least 300,000 lines:
    starts dense and sparse at whatever offsets inside blocks, waves and rounds the seed gives"""
    rng = np.random.default_rng(20261100)
    pool = NAMES + [UNKNOWN, b"chrUn_y"]
    lines, n_runs, scales, prev = [], 0, [0, 0, 0], None
    while len(lines) < 300_000:
        k = int(rng.choice(3, p=[0.6, 0.3, 0.1]))
        name = pool[int(rng.integers(0, len(pool)))]
        if name == prev:
            continue
        n = int(rng.integers(1, 2 * (1, 50, 5000)[k] + 1))
        lines += [S(name, len(lines) + j) for j in range(n)]
        n_runs += 1; scales[k] += 1; prev = name
    text = _text(lines)
    exp = _expect(text)
    assert exp[0].size == len(lines) >= 300_000 > ROUND_LINES and len(exp[6]) == n_runs > 500 and min(scales) > 40
    assert (exp[6][:, 1] == -1).sum() > 50 and (np.diff(exp[6][:, 0]) > 5000).sum() > 10
    # what this seed gives (docs/rounds/r11.md quotes these figures): another generator stream is another text, and must say so here
    assert (len(lines), n_runs, scales, int((exp[6][:, 1] == -1).sum())) == (302_624, 674, [398, 215, 61], 198)
    _check(ctx, table, text, shift=3, exp=exp)


def test_a_small_text_behind_a_large_one_on_the_same_context(ctx, table):
    """the context's scratch (tok_ws, ctg_ws) is sized by the 270,000-line text and holds its line starts, block counts and contigs; the
    small texts that follow must see none of it: k_ctg_status re-arms the line and run words, every call writes what it reads"""
    text, exp = _sparse("known")
    _check(ctx, table, text, exp=exp)
    cyc = [NAMES[i % 5] for i in range(600)]
    cid, runs = _check(ctx, table, _text([L(n, 1 + i // 5) for i, n in enumerate(cyc)]))
    assert len(runs) == 600
    cid, runs = _check(ctx, table, _text([L(n, p) for n in (b"ctgB", b"chr1", b"ctgA") for p in range(1, 301)]))
    assert runs.tolist() == [[0, 4], [300, 0], [600, 3]]
    assert _check(ctx, table, L(b"chr10", 5))[1].tolist() == [[0, 1]]
    meta, _, _ = _into(ctx, table, _text([L(b"ctgB", p) for p in range(1, 301)] + [L(b"ctgA", p) for p in range(1, 301)]))
    assert meta == [600, 1800, 0, 2]


def test_the_contigs_entry_on_a_side_stream(ctx, table):
    """stream= another stream than the current one, busy with queued work: the sizes are read behind the kernels, and the current stream
    waits for that stream before the outputs are handed back"""
    import torch
    text = _text([L(n, p) for n in (b"ctgB", b"chr1", b"ctgA") for p in range(1, 301)])
    assert len(text) > 2 * 8192
    side = torch.cuda.Stream()
    big = torch.ones(64 << 20, dtype=torch.float32, device="cuda")     # 256 MB

    def busy():
        torch.cuda.synchronize()                       # (the text is in place; nothing but the work below is in front of the call)
        with torch.cuda.stream(side):
            for _ in range(16):
                big.add_(1.0)

    cid, runs = _check(ctx, table, text, stream=side, before=busy)
    assert runs.tolist() == [[0, 4], [300, 0], [600, 3]]
    torch.cuda.synchronize()
    assert float(big[0]) == 17.0


# ---- capacities of the contigs entry point -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cap_cols,cap_bytes,cap_runs", [(16_389, 20_000, 64), (19_999, 20_000, 64), (20_000, 20_000, 64), (20_000, 19_999, 64),
                                                         (20_008, 20_064, 5), (20_000, 20_000, 4), (16_389, 19_999, 3)])
def test_capacities_of_the_contigs_entry_are_respected(ctx, table, cap_cols, cap_bytes, cap_runs):
    """20,000 lines of one column-5 byte each, five runs (79 blocks of 256 lines: two waves of the scan), into buffers longer than the
    capacities passed: nothing is written behind a capacity - pos / ref / cid / key / col_off / bases / runs keep their guard values there -,
    meta reports the lines, bytes and runs needed, the ERANGE bit is set exactly when a capacity is short, and when none is short every
    output equals its expectation.  include/nanosnp.h promises about the outputs of a call with a short COLUMN or BYTE capacity only that
    they must not be used ("with any status bit set the outputs must not be used"), so nothing is asserted about what they hold in front
    of the capacity, nor about meta[3] when the LINES were cut short (with all lines and too few bytes it is the run count still); for a short RUN capacity alone it promises "the first cap_runs
    entries were written", which is asserted"""
    starts = {0: b"ctgA", 3000: b"chr1", 3001: UNKNOWN, WAVE_LINES + 5: b"ctgB", 19_999: b"chr10"}
    text = _text(_lines_of_runs(20_000, starts))
    exp = _expect(text)
    assert exp[0].size == 20_000 > WAVE_LINES and exp[2].size == 20_000 and len(exp[6]) == 5
    meta, b, caps = _into_guarded(ctx, table, text, cap_cols, cap_bytes, cap_runs)
    for name, (cap, guard) in caps.items():
        assert b[name].shape[0] > cap and bool((b[name][cap:] == guard).all()), name
    short_text, short_runs = cap_cols < 20_000 or cap_bytes < 20_000, cap_runs < 5
    assert meta[:2] == [20_000, 20_000]
    assert bool(meta[2] & ctx.TOK_ERANGE) == (short_text or short_runs) and not meta[2] & ~ctx.TOK_ERANGE
    if cap_cols >= 20_000:
        assert meta[3] == 5                                # (the runs are found from the lines alone: a short byte capacity does not change their count)
    if not short_text:
        got = {n: t.cpu().numpy() for n, t in b.items()}
        assert np.array_equal(got["runs"][:min(cap_runs, 5)], exp[6][:cap_runs])
        if not short_runs:
            for name, e in zip(("pos", "off", "bases", "cid", "ref", "key"), exp):
                assert np.array_equal(got[name][:e.size], e), name


# ---- keys of high contig indices -----------------------------------------------------------------------------------------------------
def test_keys_of_the_highest_contig_indices(ctx):
    """a table of 2^17 names (the most the key allows), sequences of 3 to 5 bases: cid up to 131,071, key = cid << 36 | pos bit for bit.
    The table is put together from arrays (a ContigTable would copy 2^17 sequences to the device one by one)"""
    n = 1 << 17
    names = [b"n%06d" % i for i in range(n)]
    lens = 3 + np.arange(n) % 3
    seq_off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    genome = np.frombuffer(b"ACGTNacgt", np.uint8)[np.random.default_rng(77).integers(0, 9, int(seq_off[-1]))]
    seqs = [genome[a:b] for a, b in zip(seq_off[:-1].tolist(), seq_off[1:].tolist())]
    tb = type("Table", (), {"__len__": lambda self: n})()
    tb.__dict__.update(names_blob=_dev(np.frombuffer(b"".join(names), np.uint8)), name_off=_dev(np.arange(n + 1, dtype=np.int64) * 7),
                       genome=_dev(genome), seq_off=_dev(seq_off), genome_len=int(seq_off[-1]))
    lines = []
    for c, count in ((0, 60), (1, 60), (65536, 60), (-1, 30), (131070, 60), (131071, 60), (0, 1), (131071, 3)):
        name, m = (names[c], int(lens[c])) if c >= 0 else (b"n131072", 3)          # (one beyond the table: unknown)
        lines += [L(name, 1 + i % m) for i in range(count)]
    text = _text(lines)
    exp = _expect(text, names, seqs)
    cid, runs = _check(ctx, tb, text, exp=exp)
    key = exp[5]
    assert runs[:, 1].tolist() == [0, 1, 65536, -1, 131070, 131071, 0, 131071] and (key[cid < 0] == FILLER).all()
    p = int(lens[131071])
    assert p == 4 and key.max() == (131071 << 36) | p
    assert set((key[cid >= 0] >> 36).tolist()) == {0, 1, 65536, 131070, 131071}
