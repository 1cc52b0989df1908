"""nsnp_mpileup_tokenise_contigs (mpileup_tokenise.hip) through its binding, on its own: pos / col_off / bases against the oracle's
restatement of the reference's reader (oracle.mpileup_tokenise), cid / ref / key / the run table against the Python restatement of the
splitter's name rule (tests/contig_rules.py, pinned to the reference's own output by tests/test_call_mpileup_host.py) - every output bit
for bit.  The kernels' tile is 8 KB: these texts of 20-40 KB span several."""
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


def _check(ctx, table, text, shift=0):
    """every output == its expectation; shift: the text starts `shift` bytes into its device buffer"""
    import torch
    t = np.frombuffer(text, np.uint8)
    buf = torch.full((t.size + shift + 64,), ord("\n"), dtype=torch.uint8, device="cuda")      # (bytes around the text must not be looked at)
    buf[shift:shift + t.size] = _dev(t)
    pos, off, bases, ref, cid, key, runs = ctx.mpileup_tokenise_contigs(buf[shift:shift + t.size], table)
    opos, ooff, obases = oracle.mpileup_tokenise(t)
    ecid, eref, ekey, eruns = contig_rule(text, NAMES, SEQS, opos)
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


def _into(ctx, table, text, cap_runs=64):
    import torch
    d = _dev(np.frombuffer(text, np.uint8))
    cap = len(text) // 10 + 2
    mk = lambda n, dt, v: torch.full((n,), v, dtype=dt, device="cuda")
    pos, off, bases = mk(cap, torch.int64, -7), mk(cap + 1, torch.int64, -7), mk(len(text), torch.uint8, 255)
    ref, cid, key = mk(cap, torch.uint8, 255), mk(cap, torch.int32, -7), mk(cap, torch.int64, -7)
    runs = torch.full((cap_runs + 8, 2), -7, dtype=torch.int64, device="cuda")
    meta = torch.zeros(4, dtype=torch.int64, pin_memory=True)
    ctx.mpileup_tokenise_contigs_into(d, table, pos, off, bases, ref, cid, key, runs[:cap_runs], meta)
    torch.cuda.synchronize()
    return meta.tolist(), runs, (pos, ref, cid, key)


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
