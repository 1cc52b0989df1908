"""CPU side of scoring a HaplotypeModel checkpoint: the float64 rules (tests/hap_eval_rules.py) against what the reference's own code computed
(tests/golden/hap_eval.npz), the truth table and label rows against the reference's get_truth / make_train_bins (hap_truth_labels.npz), the
labelled site file, the report line and the loss quirk of evaluate_dev.py:65-66."""
from __future__ import annotations

import functools
import zlib

import numpy as np
import pytest

from nanosnp_amd import sitefile, truth
from nanosnp_amd._lib import NanoSNPError
from tests import hap_eval_rules as hr
from tests.helpers import HAP_DIMS_WEIGHTS, golden, hap_dims_cases, seeded_hap_weights

N_MAIN, SEED_MAIN = 96, 12


def main_planes():
    """the read planes behind the `main` case of hap_eval.npz: (seq, baseq, mapq, hap, ref_row) int32 for the pileup and the haplotype window,
    with an all-padding site and a depth-1 site among them.  (Seeds 500 / 600, 510 / 610 and 520 / 620 put 1, 1 and 2 of the 96 sites within
    the argmax margin of hap_eval_rules.MARGIN - more than its 1 % share: the fixture maker refused them.)"""
    from nanosnp_amd import host
    out = []
    for sd, L in ((530, 33), (630, 11)):
        planes = [a.copy() for a in host.synth_hap_planes(sd + SEED_MAIN, N_MAIN, 30, 90, L)]
        seq, bq, mq, hap, _ = planes
        seq[0], bq[0], mq[0], hap[0] = -2, -2, -2, -2
        seq[1, 1:], bq[1, 1:], mq[1, 1:], hap[1, 1:] = -2, -2, -2, -2
        out.append(planes)
    return out


def seeded_targets(seed, n, n_gt, n_zy):
    rng = np.random.default_rng(7000 + seed)
    return np.stack([rng.integers(0, n_gt, n), rng.integers(0, n_zy, n)], axis=1).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def eval_case(tag):
    """a case of hap_eval.npz with its inputs rebuilt: dict(weights, xp, xh, cls, logits, site_loss, batch_loss, batch_size, n_gt, n_zy, F).
    Inputs other than the bytes the reference module saw are an error, not a comparison against the wrong thing."""
    z = np.load(golden("hap_eval.npz"))
    if tag == "main":
        from oracle import oracle
        xp, xh = [oracle.hap_features_batch(*p, nthreads=4) for p in main_planes()]
        F, n_gt, n_zy = 105, 10, 3
        weights = seeded_hap_weights(SEED_MAIN, H=256)
        cls = seeded_targets(SEED_MAIN, N_MAIN, n_gt, n_zy)
    else:
        F, n_gt, n_zy, seed, xp, xh, _, _ = hap_dims_cases()[int(z["dims_case"])]
        weights = seeded_hap_weights(seed, F=F, n_gt=n_gt, n_zy=n_zy, **(HAP_DIMS_WEIGHTS if int(z["dims_weights_scaled"]) else {}))
        cls = seeded_targets(seed, xp.shape[0], n_gt, n_zy)
    assert [zlib.crc32(xp.tobytes()), zlib.crc32(xh.tobytes())] == z[f"{tag}_input_crc32"].tolist(), \
        f"hap_eval.npz {tag}: the rebuilt inputs are not the recorded ones"
    assert np.array_equal(cls, z[f"{tag}_cls"])
    return dict(weights=weights, xp=xp, xh=xh, cls=cls, logits=z[f"{tag}_logits"], site_loss=z[f"{tag}_site_loss"],
                batch_loss=z[f"{tag}_batch_loss"], batch_size=int(z["batch_size"]), n_gt=n_gt, n_zy=n_zy, F=F, dist=float(z[f"{tag}_dist_f64"]))


@functools.lru_cache(maxsize=None)
def eval_case_f64(tag):
    """the float64 logits of a case, computed once and shared"""
    c = eval_case(tag)
    z = hr.forward_logits_f64(c["weights"], c["xp"], c["xh"])
    z.setflags(write=False)
    return z


# ---- the labelled files of the evaluate_haplotype_bins test (tests/test_gpu_hap_eval.py; the fixture maker checks that they are admissible) ----
FILES_WEIGHTS = dict(seed=21, H=256, ih_scale=0.03, head_scale=40.0)         # genotype predictions that differ from site to site
FILES = (dict(name="ctgA_1_9.bin", n=131, seed=61, dtype="int8", mapq255=False, contig="ctgA", keep=True),
         dict(name="ctgB_1_9.bin", n=118, seed=63, dtype="int32", mapq255=True, contig="ctgB", keep=True),
         dict(name="ctgC_1_9.bin", n=53, seed=65, dtype="int8", mapq255=False, contig="ctgC", keep=False))


def file_labels(seed, n, keep=True):
    """candidate_labels of a test file: every branch of the label filter among them; keep False: no row is confident"""
    rng = np.random.default_rng(9000 + seed)
    cf = (rng.random(n) < 0.85).astype(np.int64) if keep else np.zeros(n, np.int64)
    gt = rng.choice(np.arange(-1, 12), n, p=[.02] + [.09] * 10 + [.04, .04])
    zy = rng.choice([-2, -1, 0, 1, 2, 3, 10], n, p=[.03, .35, .05, .3, .2, .04, .03])
    return np.stack([cf, gt, zy], axis=1)


def labelled_files(dirpath):
    """writes FILES with sitefile.write_haplotype_train_bin on host.synth_hap_planes, as tests/test_gpu_hap_pipeline.py::_make_bin builds
    its files -> [dict(path, refs, cands, hpos, pp, ph, labels)]"""
    import os
    from nanosnp_amd import host
    out = []
    for f in FILES:
        n, seed, contig, ref_len = f["n"], f["seed"], f["contig"], 30_000
        rng = np.random.default_rng(seed)
        pp = host.synth_hap_planes(seed, n, 30, 90, 33); ph = host.synth_hap_planes(seed + 1, n, 30, 90, 11)
        if f["mapq255"]:
            pp[2][pp[2] == 60] = 255
        seq = rng.choice(list(b"ACGTacgtN"), ref_len, p=[.23, .23, .23, .23, .02, .02, .01, .01, .02]).astype(np.uint8)
        posn = np.sort(rng.choice(np.arange(1, ref_len + 40), n, replace=False))
        posn[:2] = (3, 9)
        cands = [f"{contig}:{p}" for p in posn]
        hpos = [[f"{contig}:{max(1, p + 37 * (k - 5))}" for k in range(11)] for p in posn]
        planes = dict(zip(sitefile.HAP_PLANES, (ph[0], ph[3], ph[1], ph[2], pp[0], pp[3], pp[1], pp[2])))
        labels = file_labels(seed, n, f["keep"])
        path = os.path.join(str(dirpath), f["name"])
        sitefile.write_haplotype_train_bin(path, cands, hpos, planes, labels.astype(np.float64), plane_dtype=f["dtype"])
        out.append(dict(path=path, refs={contig: seq}, cands=cands, hpos=hpos, pp=pp, ph=ph, labels=labels))
    return out


def file_features(f):
    """the features of every row of a labelled file by the per-site host restatement of the reference rows + the oracle reduction"""
    from nanosnp_amd import host
    from oracle import oracle
    rp = host.haplotype_ref_rows(f["refs"], f["cands"], 33)
    rh = host.haplotype_ref_rows(f["refs"], f["cands"], 11, position_lists=f["hpos"])
    return oracle.hap_features_batch(*f["pp"][:4], rp, nthreads=4), oracle.hap_features_batch(*f["ph"][:4], rh, nthreads=4)


# ---- the rules against the reference's numbers ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", ["main", "dims"])
def test_rules_reproduce_the_reference_forward_and_loss(tag):
    c = eval_case(tag)
    assert c["dist"] <= 2.5e-5                                          # the maker's admissibility rule
    z64 = eval_case_f64(tag)
    assert z64.shape == c["logits"].shape == (c["xp"].shape[0], c["n_gt"] + c["n_zy"])
    assert np.abs(z64 - c["logits"]).max() <= 2.5e-5
    loss = hr.smoothed_loss(z64, c["cls"], c["n_gt"])
    assert np.abs(loss - c["site_loss"]).max() <= 1e-4
    B = c["batch_size"]
    bm = np.array([loss[a:a + B, 0].mean() + loss[a:a + B, 1].mean() for a in range(0, loss.shape[0], B)])
    assert np.abs(bm - c["batch_loss"]).max() <= 1e-4
    near = hr.margins(z64, c["n_gt"]) < hr.MARGIN
    assert near.any(1).mean() <= hr.MARGIN_SHARE
    assert ((hr.predictions(c["logits"], c["n_gt"]) == hr.predictions(z64, c["n_gt"])) | near).all()
    if tag == "dims":
        assert (c["n_gt"], c["n_zy"]) != (10, 3)


def test_label_filter_branches():
    #            cf  gt  zy
    y = np.array([[1, 0, -1],      # refcall
                  [0, 0, -1],      # not confident
                  [1, 3, 0],       # zy 0: valid, in neither list
                  [1, 3, -2],      # below valid
                  [1, 5, 1], [1, 5, 2],
                  [1, 5, 3], [1, 5, 9],     # variants by the filter; no such zygosity class
                  [1, 5, 10],      # outside valid
                  [1, 9, -1], [1, 10, -1], [1, 65, -1], [1, -1, -1],
                  [2, 1, 1]], np.int64)
    rows, cls, meta = hr.label_filter(y)
    assert rows.tolist() == [0, 4, 5, 9] and cls.tolist() == [[0, 0], [5, 1], [5, 2], [9, 0]]
    assert meta.tolist() == [4, 3, 2, 2]                                # unscorable: zy 3, zy 9, gt -1
    rows, cls, meta = hr.label_filter(y, n_gt=3, n_zy=3)
    assert rows.tolist() == [0] and meta.tolist() == [1, 6, 1, 0]


def test_single_class_head_and_out_of_range_target():
    z = np.array([[0.5, 1.0, 2.0, -1.0]])
    loss = hr.smoothed_loss(z, np.array([[0, 7]]), 1)                   # n_gt = 1: loss 0; zy target 7 counts as the last of 3
    assert loss[0, 0] == 0.0 and np.isclose(loss[0, 1], hr.smoothed_loss(z, np.array([[0, 2]]), 1)[0, 1])
    assert hr.predictions(z, 1).tolist() == [[0, 1]]


# ---- truth table and label rows ---------------------------------------------------------------------------------------------------------
def _truth_fixture():
    z = np.load(golden("hap_truth_labels.npz"))
    return z, bytes(z["fasta"]), bytes(z["bed"]), bytes(z["vcf"]), [c.decode() for c in z["candidates"]]


def test_truth_table_and_label_rows_equal_the_reference(tmp_path):
    z, fasta, bed, vcf, cand = _truth_fixture()
    fa = tmp_path / "t.fa"
    fa.write_bytes(fasta)
    table = truth.haplotype_truth_table(str(fa), bed, vcf)
    assert list(table) == ["ctgA", "ctgB"]
    labels = truth.haplotype_label_rows(table, cand)
    assert labels.dtype == np.int32 and np.array_equal(labels, z["labels"].astype(np.int32))
    for ctg, t in table.items():                                        # the whole per-contig arrays of get_truth_variants
        every = truth.haplotype_label_rows(t, [f"{ctg}:{p}" for p in range(1, len(t) + 1)])
        assert np.array_equal(every, z["table_" + ctg])
        assert t.confident.nbytes == (len(t) + 7) // 8 and t.index.size == int((z["table_" + ctg][:, 2] >= 0).sum())
    # the quirks: a BED start of 0 marks the contig's LAST base; position 0 reads it too; later truth rows win; a row outside the BED is skipped
    a = z["table_ctgA"]
    assert a[-1, 0] == 1 and a[0, 0] == 1 and a[5, 0] == 0
    assert np.array_equal(truth.haplotype_label_rows(table, ["ctgA:0"]), truth.haplotype_label_rows(table, [f"ctgA:{len(a)}"]))
    assert a[19].tolist() == [1, 9, 1] and a[9].tolist() == [0, ord("n"), -1] and a[4].tolist() == [1, 1, 2]
    # paths, files on disk and a contig selection give the same
    (tmp_path / "t.bed").write_bytes(bed); (tmp_path / "t.vcf").write_bytes(vcf)
    only_b = truth.haplotype_truth_table(str(fa), str(tmp_path / "t.bed"), str(tmp_path / "t.vcf"), contigs=["ctgB"])
    assert list(only_b) == ["ctgB"]
    assert np.array_equal(truth.haplotype_label_rows(only_b, ["ctgB:4", "ctgB:20"]), truth.haplotype_label_rows(table, ["ctgB:4", "ctgB:20"]))


def test_truth_table_raises_where_the_reference_raises():
    ref = {"c": b"ACGTACGT"}
    bed = b"c\t1\t8\n"
    row = lambda gt, ctg=b"c": ctg + b"\t2\t.\tC\tT\t9\tPASS\t.\tGT\t" + gt + b"\n"
    assert truth.haplotype_label_rows(truth.haplotype_truth_table(ref, bed, row(b"0/1")), ["c:2"]).tolist() == [[1, 6, 2]]
    with pytest.raises(NanoSNPError, match="truth VCF: contig 'x'"):
        truth.haplotype_truth_table(ref, bed, row(b"0/1", b"x"))        # a contig absent from the FASTA
    with pytest.raises(NanoSNPError, match="confident BED: contig 'x'"):
        truth.haplotype_truth_table(ref, b"x\t1\t8\n", row(b"0/1"))
    for gt in (b"./.", b"1", b"0/1/1", b"a|b"):                         # a genotype that is not two integers
        with pytest.raises(NanoSNPError, match="two integers"):
            truth.haplotype_truth_table(ref, bed, row(gt))
    with pytest.raises(NanoSNPError, match="gt21"):
        truth.haplotype_truth_table(ref, bed, b"c\t2\t.\tC\tn\t9\tPASS\t.\tGT\t0/1\n")
    with pytest.raises(NanoSNPError):
        truth.haplotype_truth_table(ref, b"c\t1\t10\n", row(b"0/1"))    # an index past the contig
    with pytest.raises(NanoSNPError):
        truth.haplotype_label_rows(truth.haplotype_truth_table(ref, bed, b""), ["c:9"])
    with pytest.raises(NanoSNPError):
        truth.haplotype_label_rows(truth.haplotype_truth_table(ref, bed, b""), ["d:1"])


# ---- the labelled site file -------------------------------------------------------------------------------------------------------------
def _planes(n, seed=5):
    from nanosnp_amd import host
    p = host.synth_hap_planes(seed, n, 20, 24, 33)
    h = host.synth_hap_planes(seed + 1, n, 20, 16, 11)
    planes = {"pileup_sequences": p[0], "pileup_baseq": p[1], "pileup_mapq": p[2], "pileup_hap": p[3],
              "haplotype_sequences": h[0], "haplotype_baseq": h[1], "haplotype_mapq": h[2], "haplotype_hap": h[3]}
    return planes


def test_labelled_site_file_round_trip(tmp_path):
    n = 7
    planes = _planes(n)
    pos = [40, 10, 30, 10, 50, 20, 60]                                  # out of order, one position twice (stable)
    cand = [f"c:{p}" for p in pos]
    hpos = [[f"c:{p + k}" for k in range(11)] for p in pos]
    labels = np.array([[1, k, (k % 4) - 1] for k in range(n)], np.float64)            # the reference's float64 rows
    path = str(tmp_path / "a.bin")
    sitefile.write_haplotype_train_bin(path, cand, hpos, planes, labels)
    order = np.argsort(np.array(pos), kind="stable")
    c2, h2, p2, y = sitefile.read_haplotype_train_bin(path)
    assert c2 == [cand[i] for i in order] and h2 == [hpos[i] for i in order]
    assert y.dtype == np.int32 and np.array_equal(np.asarray(y), labels[order].astype(np.int32))        # the labels follow their sites
    for k in sitefile.HAP_PLANES:
        assert np.array_equal(np.asarray(p2[k]), planes[k][order])
    # integer labels give the same file; a labelled file is a valid haplotype bin, and equals the unlabelled one array for array
    path_i = str(tmp_path / "i.bin")
    sitefile.write_haplotype_train_bin(path_i, cand, hpos, planes, labels.astype(np.int16))
    assert open(path, "rb").read() == open(path_i, "rb").read()
    plain = str(tmp_path / "p.bin")
    sitefile.write_haplotype_bin(plain, cand, hpos, planes)
    c3, h3, p3 = sitefile.read_haplotype_bin(path)
    c4, h4, p4 = sitefile.read_haplotype_bin(plain)
    assert c3 == c4 and h3 == h4 and all(np.array_equal(np.asarray(p3[k]), np.asarray(p4[k])) and p3[k].dtype == p4[k].dtype for k in p4)
    a, b = sitefile.read_arrays(path), sitefile.read_arrays(plain)
    assert list(a) == list(b) + ["candidate_labels"]
    with pytest.raises(sitefile.SiteFileError):
        sitefile.read_haplotype_train_bin(plain)
    # refusals
    for bad in (labels + 0.5, np.where(labels == 3, 2.0 ** 31, labels), np.where(labels == 3, np.nan, labels), labels[:, :2], labels[:-1],
                labels.astype(str)):
        with pytest.raises(sitefile.SiteFileError):
            sitefile.write_haplotype_train_bin(str(tmp_path / "bad.bin"), cand, hpos, planes, bad)
    # no site at all
    empty = {k: v[:0] for k, v in planes.items()}
    sitefile.write_haplotype_train_bin(str(tmp_path / "e.bin"), [], [], empty, np.zeros((0, 3)))
    assert sitefile.read_haplotype_train_bin(str(tmp_path / "e.bin"))[3].shape == (0, 3)


# ---- the report and the loss quirk ------------------------------------------------------------------------------------------------------
def _parts(sizes, seed=3):
    rng = np.random.default_rng(seed)
    parts = []
    for k in sizes:
        cls = np.stack([rng.integers(0, 10, k), rng.integers(0, 3, k)], 1).astype(np.uint8)
        pred = np.where(rng.random((k, 2)) < 0.7, cls, 0).astype(np.uint8)
        parts.append((rng.random((k, 2)), cls, pred))
    return parts


def test_loss_quirk_divides_by_the_batches_of_the_last_file_that_had_one():
    B = 4
    parts = _parts([10, 5])                                             # 3 batches, then 2: the divisor is 2
    res = hr.result_from(parts, B, 10, 3)
    means = [l[a:a + B, 0].mean() + l[a:a + B, 1].mean() for l, _, _ in parts for a in range(0, l.shape[0], B)]
    assert len(means) == 5 and np.isclose(res["loss"], sum(means) / 2)
    res0 = hr.result_from(parts + [(np.zeros((0, 2)), np.zeros((0, 2), np.uint8), np.zeros((0, 2), np.uint8))], B, 10, 3)
    assert np.isclose(res0["loss"], res["loss"])                        # a last file that keeps no row leaves `step` where it was
    assert np.isclose(hr.result_from(parts[::-1], B, 10, 3)["loss"], sum(means) / 3)
    acc = [(p[a:a + B, 0] == c[a:a + B, 0]).mean() for _, c, p in parts for a in range(0, c.shape[0], B)]
    assert np.isclose(res["batch_accuracy"], np.mean(acc))
    cm = res["gt_confusion"]
    assert cm.sum() == 15 and np.isclose(res["gt_accuracy"], 100.0 * np.trace(cm) / 15) and res["gt_accuracy"] > 1.0       # a percentage
    assert np.isnan(hr.result_from([], B, 10, 3)["loss"])


def test_report_line():
    from nanosnp_amd import evaluate
    res = hr.result_from(_parts([9]), 4, 10, 3)
    line = evaluate.format_haplotype_report(res)
    assert line == "AverageLoss: %.5f, GT:|Recall: %.4f, Precision: %.4f, F1: %.4f |, ACC: %.4f" % (
        res["loss"], res["gt_recall"], res["gt_precision"], res["gt_f1"], res["batch_accuracy"])
    r, p, f = evaluate._macro_prf(res["gt_confusion"])
    assert (r, p, f) == (res["gt_recall"], res["gt_precision"], res["gt_f1"])
