"""Call rows for the stage-4 group selection and its yardstick.

The yardstick shares nothing with the kernels of nanosnp_amd/csrc/pileup_groups.hip: the rows go through the library's VCF writer
(host.vcf_format_batches, the batches restarting with every contig as pipeline._format_key_rows restarts them) and the text through
merge.select_groups.  The generator is seeded and reaches every branch of the rule; `branches` names the ones a case holds, so that a test
can insist on them (tests/test_group_cuts.py).
"""
import numpy as np

from nanosnp_amd import host, merge

KEY_SHIFT = 36
MASK = (1 << KEY_SHIFT) - 1
GT_LABELS = ["AA", "AC", "AG", "AT", "CC", "CG", "CT", "GG", "GT", "TT"]
HOM_OF = {"A": 0, "C": 4, "G": 7, "T": 9}
BRANCHES = ("g>=10", "z>2", "al0_z1", "al0_z2", "two_alts_z!=2", "p_at_cut", "p_below_cut", "p_one", "p_nan", "p_zero", "p_neg_zero",
            "tail7", "tail8", "tail9", "tail10", "tail11", "tail_T", "lower_case_ref", "ref_N")


def _below(p):
    return np.nextafter(np.float32(p), np.float32(-1))


def make_case(seed, run_lengths, names=None, order=None, quality_threshold=19.0, support_quality=14.0, score_mode=host.SCORE_FLOAT64,
              batch_size=1000, support_rate=0.6, plain=False):
    """-> dict(rows float64 [N,13], ref uint8 [N], names, run_cid): the rows of len(run_lengths) contigs, run r belonging to contig order[r]
    of the table `names`; column 0 = (contig << 36) | position with ascending positions.  plain: no special probabilities and no planted
    tails (cases that are about the neighbourhoods, not the row rule)."""
    rng = np.random.default_rng(seed)
    n_runs = len(run_lengths)
    names = list(names) if names is not None else [f"ctg{i}" for i in range(n_runs)]
    order = list(order) if order is not None else list(range(n_runs))
    cuts = merge.group_cuts(quality_threshold, support_quality, score_mode)
    specials = [v for c in cuts[:2] if np.isfinite(c) for v in (c, _below(c))] + [np.float32(1.0), np.float32(np.nan), np.float32(0.0), np.float32(-0.0)]
    blocks, refs = [], []
    for r, n in enumerate(run_lengths):
        pos = np.cumsum(rng.integers(1, 50, n)) + int(rng.integers(0, 1000))
        ref = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, n)].copy()
        g = rng.integers(0, 10, n)
        z = np.where(rng.random(n) < support_rate, 2, rng.integers(0, 2, n))
        gm = np.where(rng.random(n) < 0.75, 1.0 - rng.random(n) ** 3 * 0.2, 0.4 + 0.6 * rng.random(n)).astype(np.float32)
        zm = np.where(rng.random(n) < 0.75, 1.0 - rng.random(n) ** 3 * 0.2, 0.4 + 0.6 * rng.random(n)).astype(np.float32)
        hom = rng.random(n) < 0.12                                           # the genotype is the reference letter twice: al == 0
        g[hom] = [HOM_OF[chr(c)] for c in ref[hom]]
        if not plain:
            g[rng.random(n) < 0.03] = rng.integers(10, 21, 1)[0]
            z[rng.random(n) < 0.02] = 3
            for arr in (gm, zm):
                hit = rng.random(n) < 0.10
                arr[hit] = rng.choice(specials, int(hit.sum()))
            low = rng.random(n) < 0.03
            ref[low] |= 0x20                                                 # lower case: the caller's bytes may be as the FASTA stores them
            ref[rng.random(n) < 0.01] = ord("N")
            # the last batch of the run: the genotype search of the writer runs off it when it is short (predict.py:100-131)
            tail = n - (n - 1) // batch_size * batch_size
            for j, (letter, zj) in enumerate((("T", 1), ("A", 1), ("C", 2), ("T", 2), ("G", 1))):
                at = n - 1 - j
                if at < n - tail or at < 0:
                    break
                ref[at], g[at], z[at] = ord(letter), HOM_OF[letter], zj
                gm[at], zm[at] = 0.99, (0.6, 0.95)[j & 1]
        cov = rng.integers(-40, 40, (n, 8)).astype(np.float64)
        key = (np.int64(order[r]) << KEY_SHIFT) | pos.astype(np.int64)
        blocks.append(np.column_stack([key.astype(np.float64), g, z, gm.astype(np.float64), zm.astype(np.float64), cov]))
        refs.append(ref)
    rows = np.concatenate(blocks) if blocks else np.zeros((0, 13))
    return dict(rows=np.ascontiguousarray(rows, np.float64), ref=np.concatenate(refs) if refs else np.zeros(0, np.uint8), names=names,
                run_cid=order, run_lengths=list(run_lengths), batch_size=batch_size, score_mode=score_mode, cuts=cuts)


def typed(case, a, b):
    """rows [a, b) as the typed columns the writer takes"""
    r = case["rows"][a:b]
    return dict(pos=r[:, 0].astype(np.int64) & MASK, ref=case["ref"][a:b] & 0xDF, ga=r[:, 1].astype(np.uint8), za=r[:, 2].astype(np.uint8),
                gm=r[:, 3].astype(np.float32), zm=r[:, 4].astype(np.float32), cov=r[:, 5:13].astype(np.float32))


def vcf_text(case, batch_size=None, score_mode=None):
    """the text of the rows, contig by contig in row order"""
    bs = case["batch_size"] if batch_size is None else batch_size
    mode = case["score_mode"] if score_mode is None else score_mode
    out, a = [], 0
    for cid, n in zip(case["run_cid"], case["run_lengths"]):
        t = typed(case, a, a + n)
        text, _ = host.vcf_format_batches(host.ContigTable([case["names"][cid]]), np.zeros(n, np.int32), t["pos"], t["ref"], t["ga"], t["za"], t["gm"],
                                          t["zm"], t["cov"], batch_size=bs, score_mode=mode, nthreads=1)
        out.append(text)
        a += n
    return b"".join(out).decode()


def yardstick(case, quality_threshold=19.0, adjacent_size=5, support_quality=14.0, batch_size=None, score_mode=None, nthreads=10,
              reference_bug=False):
    return merge.select_groups(vcf_text(case, batch_size, score_mode), quality_threshold, adjacent_size, support_quality, nthreads, reference_bug)


def n_groups(groups):
    return sum(len(v) for v in groups.values())


def branches(case):
    """the branches of the rule the case's rows reach (names of BRANCHES)"""
    r, ref, cuts = case["rows"], case["ref"], case["cuts"]
    g, z = r[:, 1].astype(int), r[:, 2].astype(int)
    up = ref & 0xDF
    lab = np.array([[ord(c) for c in l] for l in GT_LABELS] + [[0, 0]] * 11, np.uint8)[g]
    al = (lab[:, 0] != up).astype(int) + (lab[:, 1] != up)
    ok = (g < 10) & (z <= 2)
    p = np.concatenate([r[:, 3], r[:, 4]]).astype(np.float32)
    got = set()
    for name, cond in (("g>=10", g >= 10), ("z>2", z > 2), ("al0_z1", ok & (al == 0) & (z == 1)), ("al0_z2", ok & (al == 0) & (z == 2)),
                       ("two_alts_z!=2", ok & (al == 2) & (lab[:, 0] != lab[:, 1]) & (z != 2)),
                       ("p_at_cut", np.isin(p, cuts[:2])), ("p_below_cut", np.isin(p, [_below(c) for c in cuts[:2]])), ("p_one", p == 1.0),
                       ("p_nan", np.isnan(p)), ("p_zero", (p == 0) & ~np.signbit(p)), ("p_neg_zero", (p == 0) & np.signbit(p)),
                       ("lower_case_ref", (ref & 0x20) != 0), ("ref_N", up == ord("N"))):
        if bool(np.any(cond)):
            got.add(name)
    a = 0
    for n in case["run_lengths"]:
        tail = n - (n - 1) // case["batch_size"] * case["batch_size"] if n else 0
        if 7 <= tail <= 11:
            got.add(f"tail{tail}")
            s = slice(a + n - tail, a + n)
            if bool(np.any(ok[s] & (al[s] == 0) & (z[s] == 1) & (up[s] == ord("T")))):
                got.add("tail_T")
        a += n
    return got


TAIL_RUNS = (1007, 1008, 9, 10, 1011)                      # last batches of 7, 8, 9, 10 and 11 rows at batch_size 1000
TAIL_RUNS_10 = (27, 38, 49, 60, 7, 8, 9)                   # last batches of 7, 8, 9, 10 rows at batch_size 10, and runs that are one short batch


def default_case(score_mode=host.SCORE_FLOAT64):
    """every branch in one case: five runs whose last batch of 1000 has 7..11 rows, and one more run"""
    return make_case(20264100 + score_mode, TAIL_RUNS + (300,), batch_size=1000, score_mode=score_mode)


def short_batch_case(score_mode=host.SCORE_FLOAT64):
    return make_case(20264110 + score_mode, TAIL_RUNS_10 + (300,), batch_size=10, score_mode=score_mode)
