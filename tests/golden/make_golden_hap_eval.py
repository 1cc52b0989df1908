#!/usr/bin/env python3
"""Generate tests/golden/hap_eval.npz and tests/golden/hap_truth_labels.npz from the reference's own code.

Runs only where the reference tree is mounted (development container).  The reference's modules are imported with the stubs of SURVEY appendix
C; nothing of them is copied.

hap_eval.npz - HaplotypeModel/model_dev.LSTMNetwork.forward (:120-131) with seeded weights, per case

    main   seeded_hap_weights(12, H=256); 96 sites of features made by the reference's own dataset_dev.get_frequency_feature (+ reference row)
           from host.synth_hap_planes, as hap_fwd_large.npz builds them; seeded targets
    dims   one case of helpers.hap_dims_cases() whose (n_gt, n_zy) is not (10, 3): its inputs, seeded targets; the scaled weights of
           HAP_DIMS_WEIGHTS when they are admissible for logits, unscaled seeded weights otherwise (recorded in dims_weights_scaled)

    model(xp, xh, gt, zy) over ALL rows in one batch      -> logits fp32 [N, n_gt + n_zy]
    its two LabelSmoothingLoss(C, 0.1) on single rows     -> site_loss fp32 [N,2]
    model(...) over batches of 4, in order                -> batch_loss float64 [N / 4]

Before anything is written the float64 restatement (tests/hap_eval_rules.py) must reproduce every number, and the distance of the reference's
fp32 logits to it is recorded (dist_f64): an input is admissible for a 1e-4 test only below 2.5e-5 (the project's rule, make_golden_eval.py).
The reference's own fp32 argmax must equal the float64 argmax outside the sites whose float64 top-two margin is under 2e-4, and those may be
at most 1 % of the sites.  The inputs do not compress: the fixture holds the seeds and the CRC-32 of the feature bytes; the tests rebuild them
(tests/test_hap_eval_rules.py: eval_case) and refuse other bytes.

hap_truth_labels.npz - a small FASTA (2 contigs, lower-case and N bases), confident BED (one interval with start 0, one reaching a contig's
end), truth VCF ('/' and '|' genotypes, multi-allelic, indels, a row outside the BED, two rows on one position) and a candidate list, as bytes,
with the label rows get_truth.load_confident_bed / load_truth_vcf (-> output_labels_from_vcf_columns) leave in the per-contig arrays and
make_train_bins.py:123-127 reads out of them.  get_truth.py:266 builds the initial array with np.fromstring, which recent NumPy no longer
accepts: the array is built here with np.frombuffer, lines :267-274 restated on it.

    python tests/golden/make_golden_hap_eval.py
"""
from __future__ import annotations

import os
import sys
import tempfile
import types
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
REF = os.environ.get("REF", "/root/reference")
BATCH = 4
ADMISSIBLE = 2.5e-5
N_MAIN, SEED_MAIN = 96, 12
DIMS_CASE = 3                       # (F, n_gt, n_zy) = (96, 13, 3) of hap_fwd_dims.npz


def _stubs():
    for name, attrs in (("ranger", {"Ranger": object}), ("ranger21", {"Ranger21": object}), ("tables", {"Filters": lambda **k: None}), ("pysam", {})):
        m = types.ModuleType(name)
        for k, v in attrs.items():
            setattr(m, k, v)
        sys.modules.setdefault(name, m)
    sys.path.insert(0, os.path.join(REF, "HaplotypeModel"))


def reference_model(F, n_gt, n_zy, weights):
    import torch
    from model_dev import LSTMNetwork       # noqa: E402  (reference module)
    from utils import AttrDict              # noqa: E402
    from nanosnp_amd.fixtures import hap_weight_names
    cfg = AttrDict({"model": {"pileup_dim": F, "haplotype_dim": F, "pileup_length": 33, "haplotype_length": 11, "hidden_size": 256,
                              "lstm_layers": 3, "gt_num_class": n_gt, "zy_num_class": n_zy, "dropout": 0.1}})
    m = LSTMNetwork(cfg)
    res = m.load_state_dict({k: torch.from_numpy(w) for k, w in zip(hap_weight_names(), weights)}, strict=False)
    assert not res.unexpected_keys and all("crit" in k for k in res.missing_keys), res
    m.eval()
    return m


def main_inputs():
    """96 sites of reference-made features, as make_golden.py group_hapfwd_large builds them -> fp32 [N,105,33], [N,105,11]"""
    import dataset_dev                      # noqa: E402  (reference module)
    from tests.test_hap_eval_rules import main_planes
    xs = []
    for planes in main_planes():
        seq, bq, mq, hap, ref_row = planes
        feat = np.stack([np.concatenate([dataset_dev.get_frequency_feature(seq[i], bq[i], mq[i], hap[i]), ref_row[i][None].astype(np.float64)], 0)
                         for i in range(seq.shape[0])])
        xs.append(feat.astype(np.float32))                                                                    # predict_dev.py:35-36
    return xs


def record(tag, model, weights, xp, xh, cls, n_gt, n_zy, out):
    import torch
    from tests import hap_eval_rules as hr
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    run = lambda sl: model(t(xp[sl]), t(xh[sl]), t(cls[sl, 0].astype(np.int64)), t(cls[sl, 1].astype(np.int64)))
    with torch.no_grad():
        _, g, z = run(slice(None))
        logits = np.concatenate([g.numpy(), z.numpy()], axis=1)
        batch_loss = np.array([float(run(slice(a, a + BATCH))[0]) for a in range(0, xp.shape[0], BATCH)], np.float64)
        site_loss = np.zeros((xp.shape[0], 2), np.float32)
        for h, (crit, (r0, C)) in enumerate(zip((model.gt_crit, model.zy_crit), hr.heads_of(n_gt, n_zy))):
            for i in range(xp.shape[0]):
                site_loss[i, h] = float(crit(t(logits[i:i + 1, r0:r0 + C]), t(cls[i:i + 1, h].astype(np.int64))))
    z64 = hr.forward_logits_f64(weights, xp, xh)
    dist = float(np.abs(logits.astype(np.float64) - z64).max())
    if dist > ADMISSIBLE:
        return dist
    mine = hr.smoothed_loss(z64, cls, n_gt)
    assert np.abs(mine - site_loss).max() <= 1e-4, (tag, np.abs(mine - site_loss).max())
    bm = np.array([mine[a:a + BATCH, 0].mean() + mine[a:a + BATCH, 1].mean() for a in range(0, xp.shape[0], BATCH)])
    assert np.abs(bm - batch_loss).max() <= 1e-4, (tag, np.abs(bm - batch_loss).max())
    # the reference's own fp32 argmax against the float64 one, outside the margin rule
    near = hr.margins(z64, n_gt) < hr.MARGIN
    assert near.any(1).mean() <= hr.MARGIN_SHARE, (tag, "too many sites within the argmax margin: another seed")
    same = hr.predictions(logits, n_gt) == hr.predictions(z64, n_gt)
    assert (same | near).all(), (tag, "the reference's fp32 argmax leaves the float64 one outside the margin")
    out.update({f"{tag}_logits": logits, f"{tag}_site_loss": site_loss, f"{tag}_batch_loss": batch_loss, f"{tag}_cls": cls,
                f"{tag}_dist_f64": np.float64(dist), f"{tag}_input_crc32": np.array([zlib.crc32(xp.tobytes()), zlib.crc32(xh.tobytes())], np.int64),
                f"{tag}_near_margin": np.int64(near.any(1).sum())})
    print(f"{tag}: {xp.shape[0]} sites, |fp32 - f64| = {dist:.3e}, loss restated within {np.abs(mine - site_loss).max():.2e}, "
          f"{int(near.any(1).sum())} sites within the margin")
    return dist


def make_hap_eval():
    import torch
    from tests.helpers import HAP_DIMS_WEIGHTS, hap_dims_cases, seeded_hap_weights
    from tests.test_hap_eval_rules import seeded_targets
    torch.manual_seed(0)
    out = {"batch_size": np.int64(BATCH)}
    ws = seeded_hap_weights(SEED_MAIN, H=256)
    xp, xh = main_inputs()
    cls = seeded_targets(SEED_MAIN, N_MAIN, 10, 3)
    d = record("main", reference_model(105, 10, 3, ws), ws, xp, xh, cls, 10, 3, out)
    assert d <= ADMISSIBLE, (d, "main: not admissible: the reference's own fp32 logits are too far from float64")
    F, n_gt, n_zy, seed, xp, xh, _, _ = hap_dims_cases()[DIMS_CASE]
    assert (n_gt, n_zy) != (10, 3)
    cls = seeded_targets(seed, xp.shape[0], n_gt, n_zy)
    for scaled in (True, False):
        ws = seeded_hap_weights(seed, F=F, n_gt=n_gt, n_zy=n_zy, **(HAP_DIMS_WEIGHTS if scaled else {}))
        d = record("dims", reference_model(F, n_gt, n_zy, ws), ws, xp, xh, cls, n_gt, n_zy, out)
        if d <= ADMISSIBLE:
            break
        print(f"dims: the {'scaled' if scaled else 'unscaled'} weights are not admissible for logits (|fp32 - f64| = {d:.3e})")
    assert d <= ADMISSIBLE, (d, "dims: not admissible")
    out.update({"dims_case": np.int64(DIMS_CASE), "dims_weights_scaled": np.int64(scaled)})
    # the labelled files of the evaluate_haplotype_bins test: admissible too, and inside the margin rule?
    from tests import hap_eval_rules as hr
    from tests.test_hap_eval_rules import FILES_WEIGHTS, file_features, labelled_files
    ws = seeded_hap_weights(**FILES_WEIGHTS)
    model = reference_model(105, 10, 3, ws)
    fd, near_sites, kept = 0.0, 0, 0
    with tempfile.TemporaryDirectory() as d:
        for f in labelled_files(d):
            rows, _, _ = hr.label_filter(f["labels"])
            if not rows.size:
                continue
            xp, xh = [x[rows] for x in file_features(f)]
            with torch.no_grad():
                _, g, z = model(torch.from_numpy(xp), torch.from_numpy(xh), torch.zeros(rows.size, dtype=torch.int64), torch.zeros(rows.size, dtype=torch.int64))
            logits = np.concatenate([g.numpy(), z.numpy()], axis=1)
            z64 = hr.forward_logits_f64(ws, xp, xh)
            fd = max(fd, float(np.abs(logits - z64).max()))
            near = hr.margins(z64, 10) < hr.MARGIN
            assert ((hr.predictions(logits, 10) == hr.predictions(z64, 10)) | near).all()
            near_sites += int(near.any(1).sum()); kept += rows.size
            print("files: genotype argmax histogram", np.bincount(z64[:, :10].argmax(1), minlength=10))
    assert fd <= ADMISSIBLE, (fd, "the labelled files are not admissible: other weights")
    assert near_sites <= hr.MARGIN_SHARE * kept, (near_sites, kept)
    out.update({"files_dist_f64": np.float64(fd), "files_near_margin": np.int64(near_sites), "files_kept": np.int64(kept)})
    print(f"files: {kept} kept sites, |fp32 - f64| = {fd:.3e}, {near_sites} within the margin")
    path = os.path.join(HERE, "hap_eval.npz")
    np.savez_compressed(path, **out)
    print(f"hap_eval.npz: {os.path.getsize(path)} bytes")


# ---- hap_truth_labels.npz -------------------------------------------------------------------------------------------------------------
FASTA = (b">ctgA some description\n"
         b"ACGTNacgtnACGTTGCAacgtRYACGT\n"
         b"GGCCAATT\n"
         b">ctgB\n"
         b"ttgacaNNNNACGTACGTAC\n")
BED = (b"ctgA\t0\t6\n"            # start 0: marks index -1 (the contig's LAST base) and 0..4
       b"ctgA\t14\t22\n"
       b"ctgB\t3\t21\n")           # reaches the contig's end (index 19 is the last)
VCF = (b"##fileformat=VCFv4.2\n"
       b"#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tS\n"
       b"ctgA\t2\t.\tC\tT\t50\tPASS\t.\tGT:GQ\t0/1:30\n"
       b"ctgA\t3\t.\tG\tA\t50\tPASS\t.\tGT\t1|1\n"
       b"ctgA\t5\t.\tN\tA,C\t50\tPASS\t.\tGT\t1/2\n"                 # multi-allelic
       b"ctgA\t10\t.\tn\tG\t50\tPASS\t.\tGT\t0/1\n"                  # outside the BED: passed over
       b"ctgA\t15\t.\tT\tTGG\t50\tPASS\t.\tGT\t0|1\n"                # insertion
       b"ctgA\t16\t.\tGCA\tG\t50\tPASS\t.\tGT\t1/1\n"                # deletion
       b"ctgA\t17\t.\tC\tCA,G\t50\tPASS\t.\tGT\t1|2\n"               # insertion + SNP
       b"ctgA\t18\t.\tAa\tA,AaT\t50\tPASS\t.\tGT\t2/1\n"             # deletion + insertion
       b"ctgA\t20\t.\tC\tG\t50\tPASS\t.\tGT\t0/1\n"
       b"ctgA\t20\t.\tC\tT\t50\tPASS\t.\tGT\t1/1\n"                  # two rows on one position: the later wins
       b"ctgA\t36\t.\tT\tC\t50\tPASS\t.\tGT\t0/0\n"                  # the last base: marked through the BED start of 0
       b"ctgB\t4\t.\ta\tC,G,T\t50\tPASS\t.\tGT\t1/3\n"               # three alleles: the first two count
       b"ctgB\t20\t.\tC\tA\t50\tPASS\t.\tGT:DP\t1|0:9\n"
       b"ctgB\t2\t.\tt\tA\t50\tPASS\t.\tGT\t0/1\n")                  # outside the BED
CANDIDATES = (["ctgA:%d" % p for p in (1, 2, 3, 4, 5, 6, 7, 9, 10, 14, 15, 16, 17, 18, 19, 20, 21, 22, 23, 24, 35, 36, 0)] +
              ["ctgB:%d" % p for p in (1, 2, 3, 4, 5, 7, 10, 11, 19, 20)])


def make_truth_labels():
    import get_truth                        # noqa: E402  (reference module)
    with tempfile.TemporaryDirectory() as d:
        paths = {}
        for name, data in (("fa", FASTA), ("bed", BED), ("vcf", VCF)):
            paths[name] = os.path.join(d, "t." + name)
            with open(paths[name], "wb") as f:
                f.write(data)
        refs = get_truth.load_reference_file(paths["fa"])
        table = {}
        for ctg, seq in refs.items():
            ref = np.frombuffer(seq.encode(), np.uint8).copy()           # get_truth.py:266 with np.frombuffer; :267-274 follow
            for codes, v in (((65, 97), 0), ((67, 99), 4), ((71, 103), 7), ((84, 116), 9)):
                ref[(ref == codes[0]) | (ref == codes[1])] = v
            table[ctg] = np.zeros(shape=(len(seq), 3))
            table[ctg][:, 1] = ref
            table[ctg][:, 2] -= 1
        get_truth.load_confident_bed(paths["bed"], table)
        get_truth.load_truth_vcf(paths["vcf"], table)
    labels = []
    for pos in CANDIDATES:                                               # make_train_bins.py:123-127
        ctg, p = pos.split(":")
        labels.append(table[ctg][int(p) - 1])
    labels = np.array(labels)
    assert labels.dtype == np.float64 and (labels == np.floor(labels)).all()
    # the product's restatement reproduces every row, and the whole arrays
    from nanosnp_amd import truth
    mine = truth.haplotype_truth_table({k: v for k, v in refs.items()}, BED, VCF)
    assert np.array_equal(truth.haplotype_label_rows(mine, CANDIDATES), labels.astype(np.int32))
    for ctg, arr in table.items():
        every = truth.haplotype_label_rows(mine, ["%s:%d" % (ctg, p) for p in range(1, arr.shape[0] + 1)])
        assert np.array_equal(every, arr.astype(np.int32)), ctg
    path = os.path.join(HERE, "hap_truth_labels.npz")
    np.savez_compressed(path, fasta=np.frombuffer(FASTA, np.uint8), bed=np.frombuffer(BED, np.uint8), vcf=np.frombuffer(VCF, np.uint8),
                        candidates=np.array(CANDIDATES, dtype=np.bytes_), labels=labels,
                        **{"table_" + ctg: arr.astype(np.int32) for ctg, arr in table.items()})
    print(f"hap_truth_labels.npz: {os.path.getsize(path)} bytes; {len(CANDIDATES)} candidates, "
          f"{int((labels[:, 2] >= 0).sum())} on truth rows, {int(labels[:, 0].sum())} confident")


if __name__ == "__main__":
    _stubs()
    make_truth_labels()
    make_hap_eval()
