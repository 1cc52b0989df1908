/*
 * nanosnp.h -- C ABI of libnanosnp_hip.so: the MI355X (gfx950) implementation of NanoSNP's
 * candidate-site inference hot path.  Plain pointers and sizes only (no torch / HIP types in
 * the signatures; `stream` is a hipStream_t passed as void*, NULL = the default stream).
 *
 * The reference (huangnengCSU/NanoSNP) has no FFI of its own; each entry point replaces the
 * narrowest existing call site of the hot path (paths relative to the upstream repository):
 *
 *   nsnp_pileup_forward          LSTMNetwork.predict            PileupModel/model.py:114-119
 *                                called from                    PileupModel/predict.py:49-51
 *   nsnp_pileup_encode_columns   TensorMaker::make_tensor       dna_sv_tensor/src/make_candidate_snp_tensor/tensor_maker.cpp:61-249
 *                                + candidate test               dna_sv_tensor/src/make_candidate_snp_tensor/main.cpp:194-201
 *   nsnp_pileup_select_sites     window / pending-queue rule    dna_sv_tensor/src/make_candidate_snp_tensor/main.cpp:174-217
 *   nsnp_mpileup_tokenise        LineReader + split_line + atoll dna_sv_tensor/src/make_candidate_snp_tensor/main.cpp:162-172
 *   nsnp_mpileup_tokenise_contigs  the same + DNA_ExtractChrPileupData dna_sv_tensor/src/extract_chr_pileup_data/main.cpp:11-80
 *   nsnp_pileup_gather_windows   33-column window emission      dna_sv_tensor/src/make_candidate_snp_tensor/main.cpp:233-244
 *   nsnp_pileup_postprocess      argmax / max / depth           PileupModel/predict.py:52-65
 *   nsnp_hap_features            get_frequency_feature + ref row HaplotypeModel/dataset_dev.py:55-87,337-349
 *   nsnp_hap_forward             LSTMNetwork.predict            HaplotypeModel/model_dev.py:133-143
 *   nsnp_cat_forward             legacy CatModel.predict        HaplotypeModel/model.py:332-358 (ResCRNN: crnn.py:84-190)
 *                                called from                    HaplotypeModel/predict.py:53
 *   nsnp_cat_groups              PredictDataset.__getitem__     HaplotypeModel/dataset.py:862-915 (g0 / g1 assembly)
 *                                called from                    HaplotypeModel/predict_dev.py:35-39
 *
 * Result gather: the path's only exchange is one rooted gather of a few bytes per site at the very end.
 * PyTorch ranks do it with one torch.distributed collective (nanosnp_amd/dist.py gather_results / gather_varlen: PyTorch owns their
 * RCCL communicator and does not hand it to foreign code); callers that are not PyTorch processes use nsnp_comm_* +
 * nsnp_gather_results below, which bind a communicator of their own to the context (RCCL resolved at run time, no link dependency).
 *
 * Conventions: every pointer marked "device" is device memory owned by the caller; functions
 * are asynchronous on `stream` unless stated, return 0 on success or a negative NSNP_E* code
 * (never abort/throw; the reference's native stage abort()s, cpp_aux.cpp:10-21), and a
 * context is bound to one device and must be used by one host thread at a time.  Use one
 * context per stream when several batches are in flight.
 */
#ifndef NANOSNP_H
#define NANOSNP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NSNP_OK          0
#define NSNP_EINVAL     (-1)   /* bad argument                              */
#define NSNP_ENOMEM     (-2)   /* host or device allocation failed          */
#define NSNP_EHIP       (-3)   /* a HIP runtime call failed (see nsnp_last_hip_error) */
#define NSNP_ENOWEIGHTS (-4)   /* forward called before load_weights        */
#define NSNP_EARCH      (-5)   /* device is not gfx950                      */
#define NSNP_ESHAPE     (-6)   /* unsupported model dimensions              */
#define NSNP_ENOTSUP    (-7)   /* optional component unavailable (RCCL not found in the process or on the loader path) */
#define NSNP_ECOMM      (-8)   /* an RCCL call failed                        */

#define NSNP_PILEUP_WINDOW   33   /* PileupModel/dataset.py:11-12, 2*flanking_base+1 */
#define NSNP_PILEUP_CHANNELS 18   /* dna_sv_tensor/src/common/tensor.hpp:6-26        */
#define NSNP_GT_CLASSES      21   /* PileupModel/config/ont_pileup.yaml:17           */
#define NSNP_ZY_CLASSES       3
#define NSNP_HAP_FEATURES   105   /* HaplotypeModel/config/ont_haplotype.yaml:8-9    */

/* per-column flag bits written by nsnp_pileup_encode_columns */
#define NSNP_FLAG_PASS_AF     1u  /* pass_af as make_tensor returns it (tensor_maker.cpp:248) */
#define NSNP_FLAG_PASS_SNP    2u
#define NSNP_FLAG_PASS_INDEL  4u
#define NSNP_FLAG_CANDIDATE   8u  /* ref in ACGT && pass_af && depth >= min_coverage (main.cpp:195) */

typedef struct nsnp_ctx nsnp_ctx;

int         nsnp_version(void);
const char* nsnp_strerror(int code);
/* last hipError_t seen by this context (0 = hipSuccess) and its text; ctx == NULL reports the
 * error of the last failed nsnp_ctx_create */
int         nsnp_last_hip_error(const nsnp_ctx* ctx, const char** text);

/* Creates a context on `device` (must be gfx950).  Allocates no workspace yet. */
int nsnp_ctx_create(int device, nsnp_ctx** ctx);
int nsnp_ctx_destroy(nsnp_ctx* ctx);
/* Workspace is sized for `max_sites` sites per internal chunk (default 32768); larger calls are
 * processed in chunks.  Synchronous; call before the first forward to keep allocation out of
 * the hot loop (and out of hipGraph capture). */
int nsnp_ctx_reserve(nsnp_ctx* ctx, int64_t max_sites);

/* Options (name, value).  Unknown names / values return NSNP_EINVAL.  Precision options choose the arithmetic of the matrix
 * products (sums are fp32 in every mode):
 *   0  exact fp32 MFMA (the default: the reference computes in fp32)
 *   2  "bf16x3": every fp32 operand as three bf16 terms (8 + 8 + 8 significand bits = the full fp32 significand, fp32 exponent
 *      range: v = p0 + p1 + p2 exactly), six bf16 MFMAs per product, the three dropped cross terms below 2^-24 of the product -
 *      nothing is narrower than fp32.  Measured against a float64 evaluation of the PileupModel its error equals the fp32 path's
 *      (1-2e-6 in the probabilities); every reference golden holds the 1e-4 contract with no relaxed bound; no input range limit.
 *   1  "f16x3" (opt-in): every operand as two fp16 halves, three fp16 MFMAs per product: 21-22 significand bits per operand.
 *      DOCUMENTED BOUND: within 1e-4 of the reference on inputs whose magnitudes stay below 2048 (every pileup count, every
 *      generator-G3 feature); up to 2e-4 (measured 1.5e-4) on HaplotypeModel sites whose count-valued features reach several
 *      thousand (the saturated sites of tests/golden/hap_fwd_large.npz); caller-supplied inputs beyond +-131008 saturate.
 *      Use mode 2 where the 1e-4 contract must hold on arbitrary inputs.
 * The other options only change launch shapes.
 *   "pileup_precision"        0 fp32 (default) | 2 bf16x3 | 1 f16x3      PileupModel forward
 *   "hap_precision"           0 fp32 (default) | 2 bf16x3 | 1 f16x3      HaplotypeModel forward
 *   "cat_precision"           0 fp32 (default) | 2 bf16x3 | 1 f16x3      legacy CatModel forward
 *   "cat_conv_pix2"           1 (default) | 0                  k_cat_conv: the blocks with <= 64 output channels on 256-pixel workgroups (16 / 32 MFMAs
 *                                                              per wave between two barriers instead of 8 / 16); 0 = 128 pixels everywhere.  Same bits.
 *   "cat_conv_lds"            1 (default) | 0                  legacy CatModel 3x3 convolutions: the pixel block + halo of a channel chunk staged in
 *                                                              LDS once and read by all nine taps, or the round-3 GEMM that gathers every tap from the
 *                                                              image; the two sum the same products in a different order
 *   "hap_b3x"                 1 (default) | 0                  bf16x3 HaplotypeModel / CatModel LSTM steps: 256 x 256 workgroup tiles where the launch fills
 *                                                              the chip with them, or always the 128 x 128 tiles of the other modes (bit-identical)
 *   "hap_pass_sites"          128..131072, multiple of 128     sites per internal pass of the HaplotypeModel forward (default 16384;
 *                                                              workspace ~195 KB per site = 3.2 GB per context at the default,
 *                                                              (re)allocated synchronously by this call and by nsnp_hap_load_weights,
 *                                                              never by nsnp_hap_forward; callers with small batches or many contexts
 *                                                              set a smaller pass BEFORE loading the weights.  When the new size cannot
 *                                                              be allocated the call returns NSNP_ENOMEM and the previous pass size and
 *                                                              workspace stay in force)
 *   "recurrence_waves"        0 auto | 1/2/4/8                 waves per workgroup of the LDS-image recurrence kernels
 *   "l0_register_stationary"  2 (default) | 1 | 0             layer 0: weights in VGPRs + LDS exchange of h (1), or LDS images (0);
 *                                                              2 = on the fp32 path the kernel of 1 with its input block (integer
 *                                                              counts x fp32 weights) as exact bf16 partial products, fp32 sums;
 *                                                              in the f16x3 / bf16x3 modes 2 acts as 1
 *   "l0_site_groups"          0 auto | 1/2/4                   16-site groups per workgroup of that kernel
 *   "l1_register_stationary"  1 (default) | 2 | 0             f16x3 fused layer 1: weights in VGPRs + LDS operands as four waves x four gate
 *                                                              tiles and 16 sites per workgroup (1), as eight waves x two tiles (2), or LDS images + ring (0)
 *   "l1_site_groups"          0 auto | 2/4                     16-site groups per workgroup of the eight-wave kernel (a non-zero value selects it)
 *   "fused_l1"                1 (default) | 0                 f16x3 layer 1: projection fused into the recurrence
 *   "fused_waves"             0 auto | 4/8/12                  waves per workgroup of the fused kernel
 *   "proj1_tiles"             1..64                            row tiles per wave of the unfused projection kernel
 *   fp32 path (pileup_precision 0): "l0_register_stationary" 2 (default: the input block of layer 0 as exact bf16 partial products,
 *   16-site workgroups; "l0_site_groups" and "l0_input_weights_in_lds" shape the kernels of 1 only) | 1 | 0 (the fp32-MFMA
 *   kernels, bit-identical to each other), "l0_weave" 1 (default) | 0 (the kernel of "l0_register_stationary" 2 with the step
 *   software-pipelined - the next step's count projection is issued under this step's cell, in front of the barrier;
 *   bit-identical to 0, accepted and ignored elsewhere), "l0_prestage" 1 (default) | 0 (the kernel of "l0_weave" 1 with the
 *   workgroup's 16 windows converted once to a read-only LDS image in front of the step loop, and the loop without staging; a
 *   workgroup with a count beyond +-256 runs the loop of 0; bit-identical to 0, accepted and ignored where
 *   "l0_register_stationary" is not 2 or "l0_weave" is 0; any other value returns NSNP_EINVAL), "l1_register_stationary" 1 four waves x four gate
 *   tiles (default) | 2 eight waves x two tiles | 0 LDS-image kernels with the Xp1 round trip, "l1_site_groups" 0 | 1 | 2 | 4,
 *   "l1_stagger" 0 (default) | 1 (eight-wave kernel: waves 4-7 issue a group's next input part ahead of its cell),
 *   "l1_weave" 1 (default) | 0 (four-wave kernel, one site group: the step software-pipelined - the next step's input projection
 *   is issued in front of the barrier with the cell placed inside its MFMA burst, half of W_hh in LDS; bit-identical to 0),
 *   "head_split" 1 (default) | 0 heads with the output tiles split over eight waves, "static_priority" 0..3 (f16x3
 *   register-stationary kernels: s_setprio 1 for waves 4-7 of layer 1 / odd workgroups of layer 0; measured without effect),
 *   "l0_input_weights_in_lds" 0 (default) | 1 (fp32 layer 0, 16-site workgroups: input-part weight fragments in LDS, 128
 *   VGPRs; measured without gain).  Combinations without effect are accepted and ignored: "l1_site_groups" under
 *   "l1_register_stationary" 1 (its workgroups are always one 16-site group), "l1_stagger" outside the eight-wave kernel, "l1_weave" outside fp32 / "l1_register_stationary" 1 / one site group,
 *   "static_priority" and "fused_*" / "proj1_tiles" on the fp32 path.
 *   bf16x3 path (pileup_precision 2): "l0_site_groups" 0 auto | 1/2/4 and "l1_site_groups" 0 auto | 1/2/4 (16-site groups per
 *   workgroup of its layer-0 / layer-1 kernel); every combination returns the same bits.
 *   Every fp32 combination with the same "l0_register_stationary" class (2, or 0 / 1) returns bit-identical probabilities; the
 *   two classes differ in the low bits of the layer-0 input block (exact partial products summed in fp32 vs an fp32 fmaf chain). */
int nsnp_ctx_set_option(nsnp_ctx* ctx, const char* name, int64_t value);

/* Optional per-kernel timing: when enabled every launch of the kernels below is bracketed by a
 * HIP event pair recorded on the launch stream (up to 8192 launches per kernel between reads).
 * nsnp_ctx_read_timing waits for the recorded events, returns their summed duration and count
 * for kernel id (0 layer-0 recurrence, 1 layer-1 projection, 2 layer-1 recurrence, 3 heads,
 * 4 column encode, 5 haplotype features) and resets the counter.  Ids 6-8 bracket a whole CHAIN of launches of one
 * internal pass with one event pair each: 6 the fused LSTM step launches of a HaplotypeModel pass (83 launches of
 * k_hap_gemm), 7 the convolution GEMM + pooling launches of a CatModel pass (12 + 4), 8 a whole CatModel pass;
 * `launches` then counts passes.  Id 9: the heads launch of a HaplotypeModel pass (the softmax heads of nsnp_hap_forward or the scoring
 * heads of nsnp_hap_eval).  Ids 10-12: the forward, backward and weight-gradient launches of a chunk of nsnp_pileup_loss_grad, one event
 * pair per phase; `launches` counts chunks.  Ids 13-15: the same three phases of a chunk of nsnp_hap_loss_grad.  Synchronous. */
int nsnp_ctx_enable_timing(nsnp_ctx* ctx, int enable);
int nsnp_ctx_read_timing(nsnp_ctx* ctx, int kernel, double* total_ms, int64_t* launches);

/* Diagnostic: the shader clock (MHz) the device holds under a full-chip fp32 MFMA load of about 2 ms on `stream` (s_memtime
 * against the 100 MHz s_memrealtime in every workgroup of a probe kernel).  Boxes differ by 10 % and every MFMA fraction of a
 * bench line is priced at the 2.4 GHz peak, so the lines record it.  Synchronous; no product path depends on it. */
int nsnp_ctx_shader_clock(nsnp_ctx* ctx, double* mhz, void* stream);

/* ---- PileupModel ---------------------------------------------------------------------- */
/* host_tensors: the 24 fp32 tensors LSTMNetwork.predict uses, HOST pointers, in the
 * state-dict order of ont_pileup.chkpt (PileupModel/predict.py:212-214):
 *   encoder.lstm: l0 {w_ih[256,18], w_hh[256,64], b_ih[256], b_hh[256]}, l0_reverse {..},
 *                 l1 {w_ih[256,128], w_hh[256,64], b_ih, b_hh}, l1_reverse {..}      (16)
 *   encoder.output_proj {weight[128,128], bias[128]}                                 (2)
 *   forward_layer.dense {weight[256,128], bias[256]}                                 (2)
 *   forward_layer.genotype_layer {weight[21,256], bias[21]}, zygosity_layer {[3,256],[3]} (4)
 * Synchronous (packs and uploads the MFMA weight images). */
int nsnp_pileup_load_weights(nsnp_ctx* ctx, const float* const* host_tensors, int n_tensors);

/* x: device int32 [N,33,18] (the position_matrix of make_bin_predict_data.py:90-100; the
 * int->float conversion of predict.py:49 happens inside).  Outputs: device fp32 softmax
 * probabilities gt_prob [N,21], zy_prob [N,3] (model.py:117-118). */
int nsnp_pileup_forward(nsnp_ctx* ctx, const int32_t* x, int64_t N,
                        float* gt_prob, float* zy_prob, void* stream);

/* Same forward reading the windows straight out of the per-column count matrix:
 * site n uses counts[center_idx[n]-16 .. center_idx[n]+16][18] (no gathered copy). */
int nsnp_pileup_forward_windows(nsnp_ctx* ctx, const int32_t* counts, const int64_t* center_idx,
                                int64_t N, float* gt_prob, float* zy_prob, void* stream);

/* nsnp_pileup_forward_windows and predict.py:54-57 (np.argmax / np.max of both heads) in one call: the fp32 heads kernel writes
 * gt_arg / zy_arg (uint8) and gt_max / zy_max (fp32) from the registers that hold the probabilities, one launch less per batch than
 * forward + nsnp_pileup_postprocess; every other arithmetic mode / kernel generation runs the two back to back on `stream`.
 * Same values as the two-call sequence, bit for bit (first maximum wins, as np.argmax).  gt_arg, zy_arg, gt_max, zy_max may be device
 * pointers or pointers into PINNED HOST memory (hipHostMalloc / hipHostRegister: mapped on the device): the kernel then writes the 10
 * bytes per site straight into host memory and a streamed caller needs no D2H copy - the values are valid on the host once an event
 * recorded on `stream` behind the call has completed (nanosnp_amd/pipeline.py predict_pileup_bins). */
int nsnp_pileup_forward_windows_calls(nsnp_ctx* ctx, const int32_t* counts, const int64_t* center_idx, int64_t N,
                                      float* gt_prob, float* zy_prob, uint8_t* gt_arg, uint8_t* zy_arg,
                                      float* gt_max, float* zy_max, void* stream);

/* The call rows a streamed text run keeps on the device - rows: device float64 [N,13] = position, gt argmax, zy argmax, gt max, zy max,
 * the eight coverage channels x[n,16,{0,1,2,3,9,10,11,12}] of predict.py:63 (all exact in float64) - cut into the typed arrays the row
 * formatter (nsnp_vcf_format_batches, include/nsnp_host.h) takes.  The outputs may be device pointers or pointers into PINNED HOST memory
 * (as for nsnp_pileup_forward_windows_calls): the kernel then writes the 41 bytes per site straight into host memory and the run needs no
 * device-to-host copy at all (nanosnp_amd/pipeline.py call_contigs: its only copy-engine work is the text's way in). */
int nsnp_pileup_rows_unpack(nsnp_ctx* ctx, const double* rows, int64_t N, int64_t* pos, uint8_t* gt_arg, uint8_t* zy_arg,
                            float* gt_max, float* zy_max, float* cov8, void* stream);

/* predict.py:54-65: gt_arg/zy_arg = argmax, gt_max/zy_max = max probability,
 * depth = -(sum of the negative entries of x[n,16,{0,1,2,3,9,10,11,12}]).  All device.  depth may be NULL (then x may be too).
 * N = 0 is a no-op whatever the pointers are (an empty array has no address), as in the other calls. */
int nsnp_pileup_postprocess(nsnp_ctx* ctx, const float* gt_prob, const float* zy_prob,
                            const int32_t* x, int64_t N, uint8_t* gt_arg, uint8_t* zy_arg,
                            float* gt_max, float* zy_max, int32_t* depth, void* stream);

/* ---- pileup encode -------------------------------------------------------------------- */
/* bases: device bytes, the concatenated column-5 strings of M mpileup lines; col_off: device
 * int64 [M+1]; ref: device uint8 [M], chr_seq[pos-1] as stored in the FASTA.  Outputs (device):
 * counts int32 [M,18], depth int32 [M], flags uint8 [M] (NSNP_FLAG_*).  min_af is used for the
 * SNP and the indel test (make_predict_data.sh:120-124 passes .12 for both). */
int nsnp_pileup_encode_columns(nsnp_ctx* ctx, const uint8_t* bases, const int64_t* col_off,
                               const uint8_t* ref, int64_t M, double min_af, int min_coverage,
                               int32_t* counts, int32_t* depth, uint8_t* flags, void* stream);

/* The same with the reference program's two thresholds apart (DNA_CreateCanSnpTensor -snp_min_af / -indel_min_af, main.cpp:79-88;
 * tensor_maker.cpp:205-212: an indel allele - the I and D totals - is tested against indel_min_af, a base against snp_min_af). */
int nsnp_pileup_encode_columns2(nsnp_ctx* ctx, const uint8_t* bases, const int64_t* col_off,
                                const uint8_t* ref, int64_t M, double snp_min_af, double indel_min_af, int min_coverage,
                                int32_t* counts, int32_t* depth, uint8_t* flags, void* stream);

/* BED bitmaps (the reference's -extended_confident_bed / -confident_bed, common/bed_intv_list.cpp): one bitmap per contig, device
 * uint32 [(n_bits + 31) / 32]; bit i - the contig's 0-based base i, set by every interval [from, to) with from <= i < to - is bit (i & 31)
 * of word i >> 5 (little-endian uint32: bit i & 7 of byte i >> 3).  n_bits is the contig length.  Every bit outside [0, n_bits) reads as 0
 * (nothing is read out of bounds; the reference keeps one list over all contigs and reads the next contig's first bits there). */

/* nsnp_pileup_encode_columns2 with three additions, all optional: max_del: device int32 [M] receives the column's max_del_length
 * (main.cpp:183: the largest declared length among its counted deletions - those of declared length <= 60, one the end of the column
 * cuts short with its declared length, tensor_maker.cpp:97-103,158 - or 0); pos: device int64 [M]; conf_bits / conf_n_bits: the
 * confident bitmap - then NSNP_FLAG_CANDIDATE additionally needs a set bit in the 0-based range [pos - 1, pos + max_del_length + 1)
 * (main.cpp:194; two bits without a deletion: a site whose own base lies just left of an interval still passes).  counts, depth and the
 * other flag bits equal nsnp_pileup_encode_columns2's bit for bit; with conf_bits NULL so does NSNP_FLAG_CANDIDATE.
 * NSNP_EINVAL: conf_bits without pos, conf_bits with conf_n_bits <= 0, conf_n_bits != 0 without conf_bits. */
int nsnp_pileup_encode_columns3(nsnp_ctx* ctx, const uint8_t* bases, const int64_t* col_off,
                                const uint8_t* ref, const int64_t* pos, int64_t M, double snp_min_af, double indel_min_af,
                                int min_coverage, const uint32_t* conf_bits, int64_t conf_n_bits,
                                int32_t* counts, int32_t* depth, uint8_t* flags, int32_t* max_del, void* stream);

/* The extended-BED stage, in front of the encode (main.cpp:165-169: a line at position p is skipped unless bit p - 1 of the bitmap is set,
 * before anything else sees it): pos / col_off / bases / ref as nsnp_pileup_encode_columns takes them (M columns) -> the same four arrays
 * holding only the K kept columns, in order, bases densely repacked; none of the outputs may be its input.  Output capacities are those of
 * the inputs (pos_out, ref_out [M], off_out [M + 1], bases_out [col_off[M]]), and entries [K, M) are filled so that the unchanged encode
 * and selection over all M columns make nothing of them: empty columns (off_out[K..M] = the kept byte count), reference byte 'N',
 * position -2^62 (no step to or from it is + 1) - no count has to come back to the host between the calls.  (When NO byte is kept the
 * encode's 16-byte staging of an all-empty wave reads the 16 bytes in front of its bases: give bases_out 16 readable bytes in front, as
 * nanosnp_amd does.)  meta: int64 [4] in any memory the device can write = { K, kept bytes, kept columns in front of column own_lo, in
 * front of column own_hi }: the images of a streamed chunk's own range under the compaction (nsnp_pileup_select_sites_range_dev reads
 * them there).  Three launches; scratch lives in the context (one call at a time per context). */
int nsnp_pileup_filter_columns(nsnp_ctx* ctx, const int64_t* pos, const int64_t* col_off, const uint8_t* bases, const uint8_t* ref,
                               int64_t M, const uint32_t* bits, int64_t n_bits, int64_t own_lo, int64_t own_hi,
                               int64_t* pos_out, int64_t* off_out, uint8_t* bases_out, uint8_t* ref_out, int64_t* meta, void* stream);

/* pos: device int64 [M], the positions in line order (fold the contig index into the high bits
 * when several contigs share a call).  A site is emitted when its 33 columns are 33 consecutive
 * positions - every step + 1, as main.cpp:174-178 resets its window at any other step: positions
 * that repeat or step back (concatenated text) are taken as they come.  center_idx: device int64 [cap] receives the
 * column indices of emitted sites in ascending order; *n_sites (device int64) their number
 * (may exceed cap: then only the first cap were written). */
int nsnp_pileup_select_sites(nsnp_ctx* ctx, const int64_t* pos, const uint8_t* flags, int64_t M,
                             int64_t* center_idx, int64_t cap, int64_t* n_sites, void* stream);

/* nsnp_pileup_select_sites for one chunk of a streamed text: the same selection, and in meta (int64 [4] in any memory the device can write:
 * device or pinned host) { sites selected, how many of them lie in front of column own_lo, in front of column own_hi, sites selected } -
 * the sites the chunk OWNS (its columns without the halo lines it re-reads: main.cpp:174-217 emits a site when its last column has been
 * read) are entries [meta[1], meta[2]) of the ascending list.  No count comes back through the host. */
int nsnp_pileup_select_sites_range(nsnp_ctx* ctx, const int64_t* pos, const uint8_t* flags, int64_t M, int64_t own_lo, int64_t own_hi,
                                   int64_t* center_idx, int64_t cap, int64_t* meta, void* stream);

/* nsnp_pileup_select_sites_range with the two bounds read from memory the device can read - own: int64 [2] = { own_lo, own_hi }, e.g. meta + 2
 * of nsnp_pileup_filter_columns - when the launches run: a streamed chunk is filtered, encoded and selected without a host round trip. */
int nsnp_pileup_select_sites_range_dev(nsnp_ctx* ctx, const int64_t* pos, const uint8_t* flags, int64_t M, const int64_t* own,
                                       int64_t* center_idx, int64_t cap, int64_t* meta, void* stream);

/* The per-site values PileupModel/predict.py:52-65 hands to its row loop, as one [N,13] float64 array on the device: position, argmax of
 * the genotype / zygosity heads, their maxima, the coverage channels x[:, 16, [0, 1, 2, 3, 9, 10, 11, 12]] (predict.py:63) of the centre
 * column center_idx[n] of counts [M,18].  pos: device int64 [M]; gt_arg / zy_arg / gt_max / zy_max: device arrays of N (the outputs of
 * nsnp_pileup_forward_windows_calls). */
int nsnp_pileup_call_rows(nsnp_ctx* ctx, const int32_t* counts, const int64_t* center_idx, const int64_t* pos, const uint8_t* gt_arg,
                          const uint8_t* zy_arg, const float* gt_max, const float* zy_max, int64_t N, double* rows, void* stream);

/* The reader in front of the column encode, on the device: samtools-mpileup text resident in HBM (whole lines; the end of the
 * text ends its last line) -> per line the position, the reference byte and the column-5 string, in line order:
 *   LineReader::getline  dna_sv_tensor/src/common/line_reader.cpp:95-127  ('\n' or "\r\n" ends a line)
 *   split_line           dna_sv_tensor/src/common/cpp_aux.cpp:43-59       (tokens are maximal runs of non-tab bytes)
 *   create_pileup_tensor make_candidate_snp_tensor/main.cpp:162-172       (ref_off = atoll(token 1), pileup_bases = token 4)
 * text: device uint8 [text_len] (any alignment).  chr_seq: device uint8 [chr_len] as stored in the FASTA, with ref: device uint8
 * [cap_cols] receiving chr_seq[pos - 1] of every line (both may be NULL: no reference bytes).  pos: device int64 [cap_cols];
 * col_off: device int64 [cap_cols + 1]; bases: device uint8 [cap_bytes] - exactly the arrays nsnp_pileup_encode_columns takes.
 * meta: int64 [4] in any memory the device can write (device or pinned host memory): { lines, column-5 bytes, status, 0 }, valid when
 * the stream has passed this call.  status bits: NSNP_TOK_EFORMAT a line with fewer than five fields, NSNP_TOK_BLANK an empty or
 * CR-only line (the reference aborts on both: cpp_aux.cpp:10-21 via main.cpp:165), NSNP_TOK_EPOS a position outside [1, chr_len]
 * (main.cpp:170 asserts), NSNP_TOK_ERANGE lines > cap_cols or bytes > cap_bytes (nothing is written out of bounds; meta holds what is
 * needed).  With any status bit set the outputs must not be used.  One call at a time per context (scratch lives in the context). */
#define NSNP_TOK_EFORMAT 1
#define NSNP_TOK_BLANK   2
#define NSNP_TOK_EPOS    4
#define NSNP_TOK_ERANGE  8
int nsnp_mpileup_tokenise(nsnp_ctx* ctx, const uint8_t* text, int64_t text_len, const uint8_t* chr_seq, int64_t chr_len,
                          int64_t cap_cols, int64_t cap_bytes, int64_t* pos, int64_t* col_off, uint8_t* bases, uint8_t* ref,
                          int64_t* meta, void* stream);

/* nsnp_mpileup_tokenise for a text that holds SEVERAL contigs (samtools mpileup BAM -o pileup_data: the whole genome in one file), with
 * the contig of every line found on the device - what DNA_ExtractChrPileupData (dna_sv_tensor/src/extract_chr_pileup_data/main.cpp:11-80)
 * does on one host thread by cutting the text into <chr>.mpileup files.  text / pos / col_off / bases: as above, bit for bit what
 * nsnp_mpileup_tokenise gives on this text with chr_seq = NULL (always its three-launch form: the option tok_fused is ignored here).
 * The contig table, all device arrays: names_blob + name_off (int64 [n_contigs + 1]): the wanted names laid end to end; genome (uint8
 * [genome_len]): their sequences as stored in the FASTA, back to back; seq_off (int64 [n_contigs + 1], ascending from 0 to genome_len).
 * A line's name is the bytes in front of its first C isspace byte (main.cpp:11-19: NOT the first tab-delimited token; a line that starts
 * with a tab has the empty name); two names are equal when their bytes are.  A RUN starts at the first line and at every line whose name
 * differs from the name of the line in front; a name is looked up in the table only there (the first equal entry counts).
 *   cid  int32 [cap_cols]  the table index of the line's contig, -1 for a name the table does not hold
 *   ref  uint8 [cap_cols]  genome[seq_off[cid] + pos - 1], 'N' for cid -1
 *   key  int64 [cap_cols]  (cid << NSNP_TOK_KEY_SHIFT) | pos: the "position" nsnp_pileup_select_sites* and nsnp_pileup_call_rows take when
 *                          contigs share a call; -2^62 for cid -1 (the filler of nsnp_pileup_filter_columns: no step to or from it is + 1,
 *                          and an 'N' reference base is never a candidate)
 *   runs int64 [cap_runs][2], in any memory the device can write: { first line, cid } of every run in line order
 *   meta int64 [4], likewise: { lines, column-5 bytes, status, runs }
 * LIMITS: a key must be exact in a double (nsnp_pileup_call_rows stores it in one) and a step from a contig's last position must never
 * be + 1: n_contigs <= NSNP_TOK_MAX_CONTIGS (2^17) and genome_len < 2^NSNP_TOK_KEY_SHIFT (2^36: the table's sequences together, so
 * every contig's length, stay below 68.7 G bases) - NSNP_EINVAL otherwise.  A name may have at most NSNP_TOK_NAME_MAX bytes: a line with
 * a longer one sets NSNP_TOK_ENAME.  A name may straddle any tile boundary of the kernels.
 * status: the bits above, with NSNP_TOK_EPOS = a position outside [1, length of the line's OWN contig] on a line of a known contig (lines
 * of unknown contigs are not checked: the reference never parses them), NSNP_TOK_ERANGE also for more than cap_runs runs (meta[3] holds the
 * count needed; the first cap_runs entries were written).  Nothing is read beyond text + text_len or written beyond the capacities.
 * Eight launches, no workgroup waits for another; scratch lives in the context (one call at a time per context): 8 bytes per line of
 * min(cap_cols, text_len + 1) beside the tokeniser's. */
#define NSNP_TOK_ENAME       16
#define NSNP_TOK_KEY_SHIFT   36
#define NSNP_TOK_MAX_CONTIGS (1 << 17)
#define NSNP_TOK_NAME_MAX    255
int nsnp_mpileup_tokenise_contigs(nsnp_ctx* ctx, const uint8_t* text, int64_t text_len, const uint8_t* names_blob, const int64_t* name_off,
                                  const uint8_t* genome, const int64_t* seq_off, int64_t n_contigs, int64_t genome_len,
                                  int64_t cap_cols, int64_t cap_bytes, int64_t cap_runs, int64_t* pos, int64_t* col_off, uint8_t* bases,
                                  uint8_t* ref, int32_t* cid, int64_t* key, int64_t* runs, int64_t* meta, void* stream);

/* ---- BED region filters for a chunk that holds SEVERAL contigs (key = (cid << NSNP_TOK_KEY_SHIFT) | pos) -------------------------------
 * The bitmap TABLE lies beside the contig table of nsnp_mpileup_tokenise_contigs (same n_contigs, same seq_off), all device arrays:
 *   bed_words uint32 []               the bitmaps of all contigs, back to back
 *   bed_off   int64 [n_contigs + 1]   ascending word offsets starting at 0: contig c owns words [bed_off[c], bed_off[c + 1]), laid out as the
 *                                     single bitmaps above - bit i of the contig is bit i & 31 of its word i >> 5
 * Contig c has min(seq_off[c + 1] - seq_off[c], 32 * (bed_off[c + 1] - bed_off[c])) bits.  A contig the BED does not mention takes ZERO
 * words and every one of its bits reads 0; bits at or beyond the contig's length read 0 even where the last word has them set; nothing is
 * read outside a contig's own words, so a range that reaches past the end of contig A never sees the first bits of contig B (the reference's
 * one list over all contigs does).  A key with cid < 0 (the filler -2^62) or cid >= n_contigs never touches the table and reads 0.  bed_words
 * may be NULL when no contig owns a word.
 *
 * nsnp_pileup_filter_columns_keys = nsnp_pileup_filter_columns for keyed columns: a column stays when cid = key >> NSNP_TOK_KEY_SHIFT lies in
 * [0, n_contigs) and bit (key & (2^NSNP_TOK_KEY_SHIFT - 1)) - 1 of contig cid is set - filler keys and keys of an unknown cid are dropped
 * (they separate nothing the high bits of the kept keys do not already separate: no step between two contigs is + 1).  aux / aux_out (both
 * NULL, or device int32 [M] each): one value per column that is compacted with it, e.g. line_idx of nsnp_mpileup_line_names_contigs - the line
 * that EMITS a site is the 16th KEPT line behind its centre.  Capacities, the tail [K, M) (key -2^62, reference byte 'N', empty columns,
 * aux_out -1), meta = { K, kept bytes, image of own_lo, image of own_hi }, the 16 readable bytes in front of bases_out, the three launches and
 * the scratch in the context: as nsnp_pileup_filter_columns (the count and scatter kernels are the same templates, k_filter_scan the same
 * kernel).  NSNP_EINVAL: as there (an output that is its input, a NULL array with M > 0, n_contigs < 0, n_contigs > 0 without bed_off /
 * seq_off), and aux without aux_out or the reverse. */
int nsnp_pileup_filter_columns_keys(nsnp_ctx* ctx, const int64_t* key, const int64_t* col_off, const uint8_t* bases, const uint8_t* ref,
                                    const int32_t* aux, int64_t M, const uint32_t* bed_words, const int64_t* bed_off, const int64_t* seq_off,
                                    int64_t n_contigs, int64_t own_lo, int64_t own_hi,
                                    int64_t* key_out, int64_t* off_out, uint8_t* bases_out, uint8_t* ref_out, int32_t* aux_out, int64_t* meta,
                                    void* stream);

/* nsnp_pileup_encode_columns3 with `key` where it takes pos and the bitmap table where it takes conf_bits / conf_n_bits: with a table
 * (bed_off != NULL) NSNP_FLAG_CANDIDATE additionally needs a set bit in [p - 1, p + max_del_length + 1) of the column's OWN contig, clipped to
 * that contig's bits - a deletion at the last positions of contig A whose reach passes A's end is tested against A's bits alone; a filler
 * column or one of an unknown cid is never a candidate.  max_del is optional.  counts, depth, max_del and the other flag bits equal
 * nsnp_pileup_encode_columns2 / 3 bit for bit; without a table (bed_off NULL: bed_words must be NULL, too) so does NSNP_FLAG_CANDIDATE.
 * NSNP_EINVAL: a table without seq_off or (M > 0) without key, bed_words without bed_off, n_contigs < 0.  One launch. */
int nsnp_pileup_encode_columns_keys(nsnp_ctx* ctx, const uint8_t* bases, const int64_t* col_off, const uint8_t* ref, const int64_t* key,
                                    int64_t M, double snp_min_af, double indel_min_af, int min_coverage, const uint32_t* bed_words,
                                    const int64_t* bed_off, const int64_t* seq_off, int64_t n_contigs,
                                    int32_t* counts, int32_t* depth, uint8_t* flags, int32_t* max_del, void* stream);

/* x[n][t][c] = counts[center_idx[n]-16+t][c]; x: device int32 [N,33,18]. */
int nsnp_pileup_gather_windows(nsnp_ctx* ctx, const int32_t* counts, const int64_t* center_idx,
                               int64_t N, int32_t* x, void* stream);

/* The first two arrays of a stage-1 window file (<chr>.pd.bin; make_predict_data/main.cpp:76-127 + make_bin_predict_data.py:48-100) for
 * the N selected sites center_idx[0..N) of a chunk of M encoded columns (counts int32 [M,18], pos int64 [M], both on the device):
 *   position_matrix [N,33,18]  int16 (elem 2) or int32 (elem 4): position_matrix[n][t][c] = counts[center_idx[n] - 16 + t][c]
 *   position        [N,83]     uint8: name ':' decimal(pos[centre]) ':' then toupper(chr_seq[p - 1]) for p in [pos - 16, pos + 16] (C locale:
 *                              only a-z change), zeros up to NSNP_POSITION_WIDTH bytes
 * Both outputs and meta (int64 [4]) may lie in any memory the device can write (device or pinned host); position_matrix must be aligned to
 * 16 bytes, position to 4.  chr_seq: device uint8 [chr_len] as stored in the FASTA; name: HOST bytes, name_len of them.
 * meta = { N, overflow, status, 0 } when the stream has passed the call: overflow != 0 when elem is 2 and a value lies outside int16 (the
 * stored value is then unspecified: call again with elem 4); status != 0 when a centre lay outside [16, M - 17], a position outside
 * [0, 10^11) or a window outside the contig - the selection never hands such a site over; the kernels clamp instead of following it.
 * NSNP_EINVAL: an empty name, a NUL in it, name_len + 1 + 11 + 1 + 33 > NSNP_POSITION_WIDTH (11 digits: the longest position below
 * 2^36), elem not 2 or 4, N > 0 with M < 33.  Three launches, no scratch memory. */
#define NSNP_POSITION_WIDTH 83   /* make_bin_predict_data.py:94  StringAtom(itemsize = no_of_positions + 50) */
int nsnp_pileup_window_records(nsnp_ctx* ctx, const int32_t* counts, const int64_t* center_idx, const int64_t* pos, int64_t M, int64_t N,
                               const uint8_t* chr_seq, int64_t chr_len, const uint8_t* name, int name_len, int elem,
                               void* position_matrix, uint8_t* position, int64_t* meta, void* stream);

/* nsnp_pileup_window_records with the name of every site taken from ITS text: DNA_CreateCanSnpTensor prints column 0 of the line that
 * emits a site (make_candidate_snp_tensor/main.cpp:248: the line at centre + 16), not its contig argument.  line_idx: device int32 [M] and
 * names: device uint8 [..][NSNP_NAME_ENTRY] as nsnp_mpileup_line_names leaves them for the same lines (line_idx NULL: the entry above).
 * A name that leaves no room for 11 digits (longer than 37 bytes) sets meta[2]. */
#define NSNP_NAME_ENTRY 44       /* 40 name bytes (zero-padded), then the token's length as int32 */
int nsnp_pileup_window_records2(nsnp_ctx* ctx, const int32_t* counts, const int64_t* center_idx, const int64_t* pos, int64_t M, int64_t N,
                                const uint8_t* chr_seq, int64_t chr_len, const uint8_t* name, int name_len, int elem,
                                const int32_t* line_idx, const uint8_t* names,
                                void* position_matrix, uint8_t* position, int64_t* meta, void* stream);

/* Column 0 of every line of a chunk of mpileup text (device uint8 [text_len], whole lines, in the tokeniser's line order; a text the
 * tokeniser refuses gives nothing usable here either): line_idx[line] = -1 where the first tab-delimited token (split_line: leading tabs
 * skipped) equals `name` (HOST bytes), else the index of the entry of `names` the token was copied to (entry order means nothing).
 * meta int64 [4] (device or pinned) = { lines whose token differs, NSNP_TOK_ERANGE when they outnumber cap_names - call again with a
 * larger table -, 0, 0 }.  Four launches, no workgroup waits for another; scratch in the context: 8 bytes per 4 KB of text. */
int nsnp_mpileup_line_names(nsnp_ctx* ctx, const uint8_t* text, int64_t text_len, const uint8_t* name, int name_len, int64_t cap_lines,
                            int32_t* line_idx, uint8_t* names, int64_t cap_names, int64_t* meta, void* stream);

/* The third field of a .pd line - "<depth>-" + the column's alternative alleles as `key ' ' count ' '` in key order, right-trimmed
 * (tensor_maker.cpp:83-169, main.cpp:220-251, make_predict_data/main.cpp:88; every quirk of it: oracle/pileup_encode_oracle.c) - for the
 * same N sites, from the chunk's columns as nsnp_mpileup_tokenise leaves them (bases uint8 [n_bytes], col_off int64 [M + 1], ref uint8 [M],
 * pos int64 [M]) and the encode's depth int32 [M]; chr_seq as above.  Keys: 'I' + base + upper(allele) per distinct insertion (an allele the
 * column's end cuts short is a key of its own), 'D' + the reference bytes chr_seq[pos, pos + d) per declared deletion length d <= 60,
 * 'X' + base per mismatching base.  The first key holding a NUL - a deletion reaching past chr_len, a cut insertion - is written up to
 * that NUL, without a count, and ends the text.  Exact for any column: nothing is bounded by a list or a staged length.
 *   blob    uint8 [cap]     the texts laid end to end          (any memory the device can write)
 *   offsets int64 [N + 1]   text n is blob[offsets[n], offsets[n + 1])   (likewise)
 *   meta    int64 [4]       { bytes needed, status, 0, 0 }: status NSNP_TOK_ERANGE when needed > cap - the blob is then left untouched, the
 *                           offsets are still right
 * Four launches, no workgroup waits for another; scratch (8 bytes per site + cap) lives in the context: one call at a time per context. */
int nsnp_pileup_alt_info(nsnp_ctx* ctx, const uint8_t* bases, int64_t n_bytes, const int64_t* col_off, const uint8_t* ref, const int64_t* pos,
                         const int32_t* depth, int64_t M, const int64_t* center_idx, int64_t N, const uint8_t* chr_seq, int64_t chr_len,
                         uint8_t* blob, int64_t cap, int64_t* offsets, int64_t* meta, void* stream);

/* The three stage-1 record entries for a chunk that holds SEVERAL contigs (one whole-genome text: make_predict_data.sh:117-234 without the
 * DNA_ExtractChrPileupData pass, extract_chr_pileup_data/main.cpp:11-80).  They take the chunk's `key` (int64 [M], (cid << NSNP_TOK_KEY_SHIFT)
 * | pos as nsnp_mpileup_tokenise_contigs leaves it) where the entries above take `pos`, and the resident contig table of that call (names_blob
 * + name_off, genome + seq_off, n_contigs: device arrays; genome holds at least one readable byte) where they take chr_seq / chr_len / name.
 *
 * nsnp_pileup_window_records_keys = nsnp_pileup_window_records2 (make_predict_data/main.cpp:76-127; the name of make_candidate_snp_tensor/
 * main.cpp:248): per site cid = key[centre] >> NSNP_TOK_KEY_SHIFT, p = key[centre] & (2^NSNP_TOK_KEY_SHIFT - 1); the 33 reference bases are
 * genome[seq_off[cid] + ...], bounded by the contig's OWN length seq_off[cid + 1] - seq_off[cid]; the name is the table's name cid unless
 * line_idx[centre + 16] names an entry of `names` (nsnp_mpileup_line_names_contigs of the same lines; line_idx NULL: always the table's).
 * cap_names: the entries `names` holds - an index at or above it is treated like the "no room" entry 0x7fffffff: not followed, meta[2] set.
 *   site_key int64 [N]  key[centre] of every site (any memory the device can write, aligned to 8 bytes): the host cuts a chunk's records by
 *                       contig from it
 * meta = { N, overflow, status, 0 } as above; status != 0 also for a centre whose key is the filler or whose cid lies outside [0, n_contigs),
 * a window outside the site's own contig, a name longer than 37 bytes: all of them clamped, never followed.  The window matrix is the
 * kernel of the entries above.  Three launches, no scratch memory. */
int nsnp_pileup_window_records_keys(nsnp_ctx* ctx, const int32_t* counts, const int64_t* center_idx, const int64_t* key, int64_t M, int64_t N,
                                    const uint8_t* names_blob, const int64_t* name_off, const uint8_t* genome, const int64_t* seq_off,
                                    int64_t n_contigs, int elem, const int32_t* line_idx, const uint8_t* names, int64_t cap_names,
                                    void* position_matrix, uint8_t* position, int64_t* site_key, int64_t* meta, void* stream);

/* nsnp_mpileup_line_names against the table instead of one name: cid int32 [lines] as nsnp_mpileup_tokenise_contigs wrote it for the same
 * text (same line order).  line_idx[line] = -1 where the line's first tab-delimited token (split_line: leading tabs skipped) equals the
 * table name of cid[line], and where cid[line] < 0 (such a line never emits a site); else the index of the entry the token was copied to.
 * The CONTIG of a line follows the splitter's rule (the bytes in front of the first C isspace byte, extract_chr_pileup_data/main.cpp:11-19),
 * the name the window program prints is the tab token (make_candidate_snp_tensor/main.cpp:248): for a line "chr1 x<TAB>..." they differ, and
 * this entry keeps the position string exact ("chr1 x").  meta and the overflow rule: as nsnp_mpileup_line_names.  Four launches, no
 * workgroup waits for another; scratch in the context: 8 bytes per 4 KB of text. */
int nsnp_mpileup_line_names_contigs(nsnp_ctx* ctx, const uint8_t* text, int64_t text_len, const int32_t* cid, const uint8_t* names_blob,
                                    const int64_t* name_off, int64_t n_contigs, int64_t cap_lines, int32_t* line_idx, uint8_t* names,
                                    int64_t cap_names, int64_t* meta, void* stream);

/* nsnp_pileup_alt_info (tensor_maker.cpp:83-169, main.cpp:220-251) with key for pos and the table's genome for chr_seq: the 'D' keys read
 * genome[seq_off[cid] + p + q] only while p + q lies below the OWN contig's length and meet NUL beyond it - in a back-to-back genome the next
 * contig's bases lie right there.  A site whose key is the filler or whose cid lies outside [0, n_contigs) is a contig of length 0, and sets
 * NSNP_TOK_EPOS in the status.  blob / offsets / meta = { bytes needed, status, 0, 0 }, NSNP_TOK_ERANGE, the untouched blob, the four launches
 * and the scratch: as nsnp_pileup_alt_info. */
int nsnp_pileup_alt_info_keys(nsnp_ctx* ctx, const uint8_t* bases, int64_t n_bytes, const int64_t* col_off, const uint8_t* ref, const int64_t* key,
                              const int32_t* depth, int64_t M, const int64_t* center_idx, int64_t N, const uint8_t* genome,
                              const int64_t* seq_off, int64_t n_contigs, uint8_t* blob, int64_t cap, int64_t* offsets, int64_t* meta, void* stream);

/* ---- training labels of a chunk's selected sites (<chr>.td.bin: make_train_data/main.cpp:251-386, common/genotype.cpp:282-353) ----------
 * Per site the key of its centre, key[center_idx[n]], is looked up in truth_key (device int64 [T], ascending, no key twice).  On a hit the
 * site's code is truth_code[hit]; otherwise the homozygous-reference code of toupper(genome[seq_off[cid] + p - 1]): gt21 AA 0 / CC 4 / GG 7 /
 * TT 9, zygosity 0, both lengths 16.  A code is gt21 | zygosity << 8 | length index 1 << 16 | length index 2 << 24 (gt21 0..20 in the
 * order of GT21_LABLES, zygosity 0..2, length indices 0..32).  A site is kept when it is a truth site, when keep_thr is NULL, or when
 * (h >> 11) < keep_thr[cid] with h the splitmix64 finaliser of key + seed * 0x9E3779B97F4A7C15 (mod 2^64): a function of key and seed alone.
 *   out_center_idx int64 [N]   the centres of the kept sites, in order (device memory; may be NULL when label is NULL)
 *   label   int32 [N', 90]     one-hot rows of the kept sites: 1 at gt21, 21 + zygosity, 24 + length 1, 57 + length 2; room for N rows, 16-byte
 *                              aligned, device or pinned host memory; NULL: no row is written
 *   counts  int64 [n_contigs, 2]  device memory, or NULL: the chunk's { truth sites, other sites } per contig are ADDED to it
 *   meta    int64 [4] = { N', truth sites among N, other sites among N, status }
 * status != 0: a centre outside [0, M), a filler key, a cid outside [0, n_contigs), a position outside the site's own contig or a reference
 * byte other than A/C/G/T/a/c/g/t (the selection emits no such site) - all of them clamped, never followed.  Four launches, no workgroup
 * waits for another; scratch of its own in the context (16 bytes per site), so it may run beside the record entries on another stream. */
#define NSNP_LABEL_WIDTH 90
int nsnp_pileup_label_sites_keys(nsnp_ctx* ctx, const int64_t* key, int64_t M, const int64_t* center_idx, int64_t N, const uint8_t* genome,
                                 const int64_t* seq_off, int64_t n_contigs, const int64_t* truth_key, const uint32_t* truth_code, int64_t T,
                                 const uint64_t* keep_thr, uint64_t seed, int64_t* out_center_idx, int32_t* label, int64_t* counts,
                                 int64_t* meta, void* stream);

/* ---- scoring a checkpoint on training windows (PileupModel/train.py:93-150, its eval()) -------------------------------------------------
 * fp32 only: with pileup_precision 1 or 2 every entry of this block that runs the network returns NSNP_EINVAL.  Head rows at the ABI, as the
 * label row of a <chr>.td.bin orders them: 0-20 genotype, 21-23 zygosity, 24-56 indel1, 57-89 indel2.
 *
 * nsnp_pileup_load_indel_heads: host_tensors = { indel1_layer.weight [33,256], .bias [33], indel2_layer.weight [33,256], .bias [33] } (n >= 4),
 * valid only after nsnp_pileup_load_weights (NSNP_ENOWEIGHTS before); packs the six-tile image of all 90 head rows.  A later
 * nsnp_pileup_load_weights invalidates it. */
int nsnp_pileup_load_indel_heads(nsnp_ctx* ctx, const float* const* host_tensors, int n);

/* The classes of label rows (PileupModel/dataset.py:78-82,98-104): per family the index of the first maximum of its slice (np.argmax; an
 * all-zero slice gives 0).  With variants_only != 0 only rows of zygosity class > 0 are kept.  Kept rows, compacted and in their order:
 *   cls        uint8 [N,4]   { gt, zy, id1, id2 }                       (device)
 *   center_idx int64 [N]     33 * n + 16 of row n: the centre of its window in a pass flattened to [N * 33, 18]   (device)
 *   meta       int64 [4]   = { kept, rows of N that are not one-hot in some family, status (always 0), 0 }; device or pinned host memory
 * Nothing is written behind the kept rows.  Three launches (flags, one-workgroup exclusive scan, compaction), no workgroup waits for
 * another; scratch of its own in the context (12 bytes per row). */
int nsnp_pileup_label_classes(nsnp_ctx* ctx, const int32_t* label, int64_t N, int variants_only, uint8_t* cls, int64_t* center_idx,
                              int64_t* meta, void* stream);

/* LSTMNetwork.forward without its loss (PileupModel/model.py:97-100,66-73): layers 0 and 1 as nsnp_pileup_forward_windows launches them, then
 * all four heads as raw logits, fp32 [N,90].  center_idx NULL: counts is [N,33,18].  NSNP_ENOWEIGHTS without the indel heads. */
int nsnp_pileup_forward_logits(nsnp_ctx* ctx, const int32_t* counts, const int64_t* center_idx, int64_t N, float* logits, void* stream);

/* The same forward with the label-smoothed loss (PileupModel/optim.py:137-144 before its mean), the argmax and the confusion counts in the heads
 * kernel.  cls uint8 [N,4]: the target classes (a class outside its head counts as the head's last).  Per site and head h with C classes:
 *   lp = z - logsumexp(z);  site_loss[n,h] = -(0.9 lp[t] + 0.1 / (C - 1) (sum(lp) - lp[t]));  pred[n,h] = first maximum of z
 *   counters int64 [NSNP_EVAL_COUNTERS]: four matrices [target][predicted], 21x21, 3x3, 33x33, 33x33 back to back; ADDED to (device memory)
 *   logits   NULL, or fp32 [N,90]: with NULL no logit reaches memory. */
#define NSNP_EVAL_COUNTERS 2628
int nsnp_pileup_eval_windows(nsnp_ctx* ctx, const int32_t* counts, const int64_t* center_idx, const uint8_t* cls, int64_t N, float* site_loss,
                             uint8_t* pred, int64_t* counters, float* logits, void* stream);

/* The two entries above with the arithmetic as an argument: precision 0 (exact fp32), 1 (f16x3), 2 (bf16x3), or -1 for the context's
 * pileup_precision.  The entries above are fp32 only and return NSNP_EINVAL while the context option is 1 or 2; these neither read (unless
 * -1) nor set the option.  precision 0 runs the implementation of the entries above: the same bytes.  Under 1 and 2 a scoring pass runs the
 * layer kernels nsnp_pileup_forward_windows runs in that arithmetic under the context's options and differs from it in the heads launch
 * only: the accumulators of the genotype and zygosity rows are the bits that forward takes its softmax from, and the tail (loss, first
 * argmax, counters) is the fp32 entry's, operation for operation.  No float is added atomically; a second run gives the same bytes.
 * NSNP_EINVAL for NULL pointers or a precision outside -1..2, NSNP_ENOWEIGHTS without the indel heads, nothing written either way;
 * N == 0 is a no-op.  (A first bf16x3 pass on a context whose workspace was reserved for another arithmetic re-reserves it, synchronously.) */
int nsnp_pileup_forward_logits2(nsnp_ctx* ctx, const int32_t* counts, const int64_t* center_idx, int64_t N, int precision, float* logits,
                                void* stream);
int nsnp_pileup_eval_windows2(nsnp_ctx* ctx, const int32_t* counts, const int64_t* center_idx, const uint8_t* cls, int64_t N, int precision,
                              float* site_loss, uint8_t* pred, int64_t* counters, float* logits, void* stream);

/* Test tap: runs the layer launches of the PileupModel forward in arithmetic `precision` (0, 1, 2, or -1 for the context's
 * pileup_precision) under the context's current options - the same kernels on the same workspace as nsnp_pileup_forward /
 * nsnp_pileup_forward_logits2 - then, in place of the heads launch, ONE un-tiling launch that writes the named image to `out` as plain
 * fp32 in natural order, and returns.  counts / center_idx as nsnp_pileup_forward_logits (center_idx NULL: counts is [N,33,18]).
 *   stage                 image                                                         out
 *   NSNP_PILEUP_ST_H0     h of layer 0 at all 33 positions, feature = dir * 64 + unit   [N,33,128]  (torch's bidirectional output)
 *   NSNP_PILEUP_ST_H1C    h of layer 1 at position 16, [h_fwd ; h_bwd]                  [N,128]
 * The storage of each arithmetic is decoded: the unit order of the fp32 rows ([site][t][dir][q][16], unit 4 i + q at entry i of row q),
 * an f16x3 (hi, lo) pair as hi + lo, the three bf16 planes of the bf16x3 H0 (16-site groups) as their exact sum.  Only sites < N are
 * written.  One pass: 0 < N <= the reserved chunk (nsnp_ctx_reserve, 32768 by default); out_floats must be the image's size exactly.
 * NSNP_EINVAL otherwise (also for a NULL pointer, an unknown stage or precision), nothing launched. */
#define NSNP_PILEUP_ST_H0   0
#define NSNP_PILEUP_ST_H1C  1
#define NSNP_PILEUP_N_STAGES 2
int nsnp_pileup_forward_stage(nsnp_ctx* ctx, const int32_t* counts, const int64_t* center_idx, int64_t N, int precision, int stage,
                              float* out, int64_t out_floats, void* stream);

/* batch_sum[b,h] = the float64 sum of site_loss[n,h] over the rows n of batch b (rows b * batch_size ..), double [ceil(N / batch_size), 4]: one
 * workgroup per batch, a fixed tree - the same bits whatever the launch and the run.  The caller divides by the batch's size. */
int nsnp_pileup_batch_loss(nsnp_ctx* ctx, const float* site_loss, int64_t N, int64_t batch_size, double* batch_sum, void* stream);

/* ---- training the PileupModel: the sample list of a pass under balance_dataset upsampling (PileupModel/dataset.py:32-66, use_balance) ------
 * cls uint8 [N,4]: the rows' classes { gt, zy, id1, id2 } as nsnp_pileup_label_classes leaves them, device.
 *   samples int64 [cap]  row indices in [0, N); the first M are written, nothing behind them                                 (device)
 *   sizes   int64 [63]   rows per category, or NULL                                                                          (device)
 *   meta    int64 [8]  = { M, K, U, max, rows in no category, status (0, or 1 when U == 0), 0, 0 }; device or pinned host memory
 * The rule.  The category of a row is c = 3 gt + zy (gt 0..20, zy 0..2), the categories stand in ascending c (the insertion order of the
 * reference's dict).  A row with gt >= 21 or zy >= 3 is in no category (the reference's np.where matches nothing for it): it is counted and
 * never sampled.  size[c] = the rows of c, max = the largest size, K = the categories with size > 0, U = those with 0 < size < max - the
 * reference's non_zero_categories, which does NOT count the categories that already stand at max: that quirk is kept.  Every nonempty
 * category owns max slots: slot r < size[c] holds the category's r-th row in row order, slot r >= size[c] a row drawn with replacement from
 * the category's own rows, once per slot.  The balanced list has L = K max slots, and M = L / U (integer division: int(L / U) of
 * dataset.py:65 for every L < 2^38 and U <= 62) samples are drawn with replacement from the slots.  The reference's shuffle in front of that
 * draw does not change its distribution and is not made.
 * U == 0 - N == 0, one category, or every nonempty category at the same size - is where the reference divides by zero.  Here it is an
 * ordinary event (the last pass of a file may hold one row): status 1, M = 0, no sample written, sizes and meta written; the caller trains
 * such a pass on its rows as they are.
 * The bound.  M <= 2 N always: E >= 1 categories stand at max, so max <= N / E, U = K - E, and K / (E (K - E)) <= K / (K - 1) <= 2 for
 * K >= 2.  A buffer of 2 N entries always suffices.
 * The draws (csrc/nsnp_philox.hpp; key { seed & 0xffffffff, seed >> 32 }; index(r, n) = ((uint64)r * n) >> 32).  Sample m takes the words v
 * of Philox4x32-10 at counter { m & 0xffffffff, m >> 32, draw, 0 }: its category is the k-th nonempty one, k = index(v[0], K), its slot
 * r = index(v[1], max) - a uniform slot of K max is a uniform category times a uniform slot within it, as every category owns max slots.
 * An upsampled slot (c, t = r - size[c]) holds the category's row number index(w[0], size[c]), w at counter { t, c, draw, 1 }: two samples
 * that hit the same slot get the same row, as in the reference.  The reference's np.random is unseeded, so only the distribution is its
 * own; here the list is a pure function of (cls, seed, draw), the same bits on every run whatever the grid.  `draw` is the caller's pass
 * counter.  The scope is the N rows of the call - a pass - where the reference's is a file.
 * NSNP_EINVAL with nothing written: cap < M, N < 0 or N >= 2^32, samples NULL with M > 0.
 * Four launches: the rows of every block of 256 per category (32-bit integer adds in LDS, whose order cannot reach the sums); ONE workgroup
 * that scans the blocks' counts per category, serially per lane over a run of blocks, and makes the plan (sizes, offsets, max, K, U, M,
 * the table of nonempty categories); every block ranks its rows inside their categories by ballots, stably, and writes the sorted list;
 * placement, a lane per sample, which also writes sizes and meta.  No workgroup waits for another and no float is involved.  Between the
 * third and the fourth the entry WAITS for the stream once and reads M: cap cannot be held against M without it.  With N == 0 there are two
 * launches and no wait (status 1).  Scratch: nsnp_pileup_label_classes' buffer, 1,600 bytes + 256 per block of 256 rows + 4 per row (the
 * plan, the counts, the list), grown as there; it is overwritten, so run the entry behind the work that reads a label pass's scratch - on
 * the same stream, or after it has finished. */
int nsnp_pileup_balance_samples(nsnp_ctx* ctx, const uint8_t* cls, int64_t N, uint64_t seed, uint32_t draw, int64_t* samples, int64_t cap,
                                int64_t* sizes, int64_t* meta, void* stream);

/* ---- training the PileupModel: the loss gradients of a batch (PileupModel/train.py:56-59, model(...) and loss.backward()) ---------------
 * fp32 only and one device: with pileup_precision 1 or 2 nsnp_pileup_loss_grad returns NSNP_EINVAL.  The entries need no
 * nsnp_pileup_load_weights: the parameters are the caller's device tensors in plain state-dict layout, because they change every step; the
 * packed images of the inference entries are not read and not refreshed (upload a trained state again to score or call with it).
 *
 * nsnp_pileup_train_reserve allocates the workspace of the saved activations and gate gradients, about 194 KB per site (rounded up to 16
 * sites) plus 128 KB per 1,024 (site, step) rows; synchronous.  NSNP_ENOMEM: the previous reservation stays in force.  A batch larger than
 * the reservation runs in chunks of that size, in order, adding into the same gradients.
 *
 * nsnp_pileup_loss_grad, asynchronous on `stream`:
 *   params     HOST array of 24 DEVICE pointers, the tensors, order and shapes of nsnp_pileup_load_weights
 *   counts, center_idx, cls   as nsnp_pileup_eval_windows takes them (center_idx NULL: counts is [N,33,18]); cls uint8 [N,4], columns 0
 *              (genotype) and 1 (zygosity) used, a class outside its head counts as the head's last
 *   keep_mask  NULL (no dropout), or device uint8 [N,33,128] of 0 / 1 in h0's order [forward 64 | reverse 64]: layer 1 sees
 *              h0 * keep_mask * keep_scale (keep_scale = 1 / (1 - p) of nn.LSTM(dropout=p)), the backward pass applies the same factor
 *   grads      HOST array of 24 device pointers, same shapes: OVERWRITTEN with d(mean gt loss + mean zy loss) / d(param), the means over all
 *              N sites.  bias_ih and bias_hh of a layer and direction receive the same values.  The indel heads are not in the loss.
 *   site_loss  NULL, or device fp32 [N,2]: the label-smoothed losses of nsnp_pileup_eval_windows, genotype and zygosity
 *   pred       NULL, or device uint8 [N,2]: the first maximum of the genotype / zygosity logits
 * N == 0 is a no-op (grads untouched).  NSNP_EINVAL for null arguments and without a reservation.  The network runs the reduced schedule
 * of the inference entries (layer 1: 17 steps per direction, dense layers and heads at position 16), which is exact for the gradient too
 * because the loss reads position 16 only.  Every matrix product is fp32 MFMA; no floating-point atomics: the same call gives the same
 * bits twice.  nsnp_ctx_read_timing ids 10, 11, 12: the forward, backward and weight-gradient phases of a chunk, one event pair each. */
int nsnp_pileup_train_reserve(nsnp_ctx* ctx, int64_t max_sites);
int nsnp_pileup_loss_grad(nsnp_ctx* ctx, const float* const* params, const int32_t* counts, const int64_t* center_idx, const uint8_t* cls,
                          int64_t N, const uint8_t* keep_mask, float keep_scale, float* const* grads, float* site_loss, uint8_t* pred,
                          void* stream);

/* ---- training: the optimiser step (PileupModel/train.py:61-62, clip_grad_norm_ and optimizer.step(); optim.py:67-84, radam.py, lookahead.py) ----
 * Generic over tensors: nothing here knows the PileupModel.  nsnp_optim_step, asynchronous on `stream`, two launches, no allocation, no host
 * synchronisation, no floating-point atomics (the same call on the same bits gives the same bits):
 *   params, grads, exp_avg, exp_avg_sq, slow   HOST arrays of n_tensors (1..NSNP_OPTIM_MAX_TENSORS) DEVICE pointers to fp32 tensors of counts[i] >= 1
 *              floats each; any 4-byte alignment (views into one flat buffer are fine; 16-byte accesses are used only where all of a tensor's
 *              pointers allow them, with the same bits either way).  grads is only read.  slow (and every slow[i]) may be NULL when args->sync
 *              is 0.  Tensors must not overlap.
 *   args       the scalars of this step, computed by the caller in float64 as the reference's Python does:
 *                max_norm      > 0: gradients are scaled by c = min(1, max_norm / (norm + 1e-6)), norm the L2 norm over all tensors
 *                              (torch.nn.utils.clip_grad_norm_); <= 0: no clipping
 *                wd_mode       0 none; 1 g += weight_decay * p (torch Adam's L2 form); 2 p += decay * p in front of the update (radam.py:69-70,
 *                              decay = -weight_decay * lr)
 *                beta1, beta2  in [0, 1):  m = beta1 m + (1 - beta1) g,  v = beta2 v + (1 - beta2) g g
 *                form          0: p -= a * m / (sqrt(v) * b + eps);  1: p -= a * m
 *                              Adam:  form 0, a = lr / (1 - beta1^t), b = 1 / sqrt(1 - beta2^t)
 *                              RAdam: b = 1, a = step_size * lr, form 0 when N_sma >= 5 and form 1 below (radam.py:55-67,73-77)
 *                sync          0 none; 1 a Lookahead sync: slow += alpha * (p - slow), p = slow (alpha in [0, 1]); 2 the first sync: slow = p
 *   scratch    device fp32 [nsnp_optim_scratch_floats(n_tensors, counts)]: the per-workgroup sums of g * g; needed when max_norm > 0 or
 *              grad_norm_out is given, may be NULL otherwise (the first launch is skipped then)
 *   grad_norm_out  NULL, or one device fp32: the unclipped norm
 * NSNP_EINVAL, with nothing launched, for a null pointer, n_tensors outside 1..64, a count below 1, a pointer that is not 4-byte aligned, beta1 or
 * beta2 outside [0, 1), alpha outside [0, 1], form / wd_mode / sync outside their lists.
 * nsnp_optim_scratch_floats: the floats of scratch for these counts (>= 1), or NSNP_EINVAL; no device is touched. */
#define NSNP_OPTIM_MAX_TENSORS 64
typedef struct nsnp_optim_args {
    double max_norm, weight_decay, decay, beta1, beta2, eps, a, b, alpha;
    int wd_mode, form, sync;
} nsnp_optim_args;
int64_t nsnp_optim_scratch_floats(int n_tensors, const int64_t* counts);
int nsnp_optim_step(nsnp_ctx* ctx, int n_tensors, float* const* params, const float* const* grads, float* const* exp_avg,
                    float* const* exp_avg_sq, float* const* slow, const int64_t* counts, const nsnp_optim_args* args, float* scratch,
                    float* grad_norm_out, void* stream);

/* The other optimiser types of the reference's build_optimizer (PileupModel/optim.py:42-104): Novograd (novograd.py:197-221; amsgrad and
 * grad_averaging off, as optim.py builds it), torch.optim.SGD (dampening 0) and torch.optim.Adadelta, each behind the same clip and in front of
 * the same Lookahead sync.  The contract of nsnp_optim_step: asynchronous on `stream`, two launches, no allocation, no host synchronisation, no
 * floating-point atomics, grads only read, any 4-byte alignment with the same bits.
 *   state_a, state_b   HOST arrays of DEVICE pointers like params, used or ignored (NULL allowed) by kind:
 *                        NSNP_OPTIM_NOVOGRAD   state_a exp_avg;  state_b ignored.  The second moment is ONE fp32 per tensor: layer_in[n_tensors]
 *                                              (device, read) and layer_out[n_tensors] (device, written; a different array: swap the two behind
 *                                              every step, start from zeros).  n_t = the squared norm of tensor t's clipped gradient;
 *                                              v_t = (v_t == 0) ? n_t : beta2 v_t + (1 - beta2) n_t at every step;  x = g c / (sqrt(v_t) + eps);
 *                                              x += weight_decay p;  m = beta1 m + x;  p -= lr m.  scratch is always needed.
 *                        NSNP_OPTIM_SGD        state_a momentum_buffer, ignored when momentum == 0;  state_b ignored.  x = g c + weight_decay p;
 *                                              buf = momentum buf + x (from zeros: torch's first step);  x = nesterov ? x + momentum buf : buf;
 *                                              p -= lr x.
 *                        NSNP_OPTIM_ADADELTA   state_a square_avg, state_b acc_delta.  x = g c + weight_decay p;  sq = rho sq + (1 - rho) x x;
 *                                              delta = sqrt(acc + eps) / sqrt(sq + eps) x;  acc = rho acc + (1 - rho) delta delta;  p -= lr delta.
 *                      layer_in / layer_out are ignored by the other two kinds.  max_norm, sync, alpha, slow, scratch, grad_norm_out: as above
 *                      (nsnp_optim_scratch_floats sizes scratch for both entries).
 * NSNP_EINVAL, with nothing launched, for a null or not 4-byte aligned pointer that the kind uses, n_tensors outside 1..64, a count below 1, an
 * unknown kind, beta1 / beta2 / rho / momentum outside [0, 1) (whatever the kind: leave the unused ones 0), alpha outside [0, 1], nesterov
 * outside 0 / 1 or set with momentum == 0 (as torch refuses it), sync outside its list, Novograd without scratch or without both layer arrays,
 * layer_in == layer_out. */
#define NSNP_OPTIM_NOVOGRAD 0
#define NSNP_OPTIM_SGD 1
#define NSNP_OPTIM_ADADELTA 2
typedef struct nsnp_optim_kind_args {
    double lr, beta1, beta2, eps, weight_decay, momentum, rho, alpha, max_norm;
    int kind, nesterov, sync;
} nsnp_optim_kind_args;
int nsnp_optim_step_kind(nsnp_ctx* ctx, int n_tensors, float* const* params, const float* const* grads, float* const* state_a,
                         float* const* state_b, float* const* slow, const int64_t* counts, const nsnp_optim_kind_args* args,
                         const float* layer_in, float* layer_out, float* scratch, float* grad_norm_out, void* stream);

/* ---- HaplotypeModel ------------------------------------------------------------------- */
/* seq/bq/mq/hap: device int32 [N,D,L] planes as write_to_bins.py:44-61 stores them (padding
 * rows are -2); ref_row: device int32 [N,L].  out: device fp32 [N,105,L] -- float64 math as
 * numpy does, then the fp32 cast of predict_dev.py:35-36. */
int nsnp_hap_features(nsnp_ctx* ctx, const int32_t* seq, const int32_t* bq, const int32_t* mq,
                      const int32_t* hap, const int32_t* ref_row, int64_t N, int D, int L,
                      float* out, void* stream);

/* The same reduction on int8 read planes (every value of the four planes fits: base codes -2..4, HP -2..3, base
 * quality <= 93, mapping quality <= 60 with -2 as padding): a quarter of the bytes over PCIe and from HBM.  Results are
 * bit-identical to nsnp_hap_features on the widened planes.  ref_row stays int32 [N,L]. */
int nsnp_hap_features_i8(nsnp_ctx* ctx, const int8_t* seq, const int8_t* bq, const int8_t* mq, const int8_t* hap,
                         const int32_t* ref_row, int64_t N, int D, int L, float* out, void* stream);

/* Read arrangement of the stage-4 generator (create_pileup_haplotype.py:140-207, write_to_bins.py:15-61):
 * per site keep the reads whose base at the centre column is non-zero, order them by the HP tag at
 * the centre column (ties keep input order), pad with -2 to D_out rows, cut at D_out.  Inputs are
 * device int32 [N,R,L] read matrices (n_reads[N] valid rows each, NULL = all R); outputs device int32
 * [N,D_out,L] planes in the layout nsnp_hap_features consumes; depth[N] (optional) = rows kept. */
int nsnp_hap_arrange_reads(nsnp_ctx* ctx, const int32_t* seq, const int32_t* bq, const int32_t* mq,
                           const int32_t* hap, const int32_t* n_reads, int64_t N, int R, int L, int D_out,
                           int32_t* oseq, int32_t* obq, int32_t* omq, int32_t* ohap, int32_t* depth, void* stream);

/* The same with a choice of the order among reads with equal centre HP (the reference sorts with pandas' default quicksort,
 * numpy.argsort(kind="quicksort"); the order among ties decides which reads a D_out cut keeps and the row order of every bin):
 *   NSNP_TIE_STABLE  ties keep their input order (nsnp_hap_arrange_reads).  No numpy build is claimed: the reference's bins equal
 *                    these up to the order inside each HP group, and at sites deeper than D_out up to which reads are kept.
 *   NSNP_TIE_NUMPY1  NumPy 1.x's scalar introsort (aquicksort_ with its aheapsort_ fallback), exactly: the order of NumPy 1.24
 *                    and earlier on every CPU - the reference's environment - and of later NumPy with SIMD sort dispatch disabled.
 *                    With the rows in the order the reference first sees the reads, the planes equal its bins row for row.
 * NumPy 1.25 and later with AVX-512 or AVX2 sort dispatch follow a CPU-dependent order that neither mode claims.
 * Any other tie_order is NSNP_EINVAL.  Both modes accept the same shapes (NSNP_ESHAPE beyond 64 KB of LDS: 2R + D_out + 1 words). */
#define NSNP_TIE_STABLE 0
#define NSNP_TIE_NUMPY1 1
int nsnp_hap_arrange_reads2(nsnp_ctx* ctx, const int32_t* seq, const int32_t* bq, const int32_t* mq,
                            const int32_t* hap, const int32_t* n_reads, int64_t N, int R, int L, int D_out, int tie_order,
                            int32_t* oseq, int32_t* obq, int32_t* omq, int32_t* ohap, int32_t* depth, void* stream);

/* ---- stage-4 read matrices from decoded alignment records (create_pileup_haplotype.py:39-60,89-134) -------------------------------------
 * The records of ONE contig as a struct of arrays on the device, in file (coordinate) order:
 *   start     int64 [R]      1-based leftmost reference position, non-decreasing
 *   mapq      uint8 [R]      hp  int32 [R]  the HP tag, -1 = no tag (counts as 3)
 *   cigar     uint32 [sum n_ops]  BAM's encoding len << 4 | op, ops 0..8 = MIDNSHP=X;  cigar_off int64 [R+1]
 *   seq, qual uint8 [sum query_len]  one ASCII base / one quality per base, soft clips included;  seq_off int64 [R+1]
 * cols int64 [P]: the wanted 1-based columns, strictly increasing.  A record covers [a, b], b = a + (sum of M, D, N, =, X lengths) - 1.
 * The callers validate the arrays on the host (readmatrix.AlignmentRecords); the kernels never read a base outside a record's own
 * seq range whatever the CIGAR says (such a cell counts as a foreign base).
 *
 * scratch: nsnp_hap_read_scratch_bytes(R, P) bytes of device memory, 16-byte aligned, the caller's (0 = R or P out of range).
 *
 * nsnp_hap_read_depths: depth[c] int32 [P] = records with a <= cols[c] <= b (deletions and reference skips count, as pysam's
 * PileupColumn.n does); rows (optional, device int64 [1]) = records that cover at least one column.  Integer atomics into a
 * difference array and a prefix sum: no result depends on an order.
 *
 * nsnp_hap_read_matrices: the four int32 matrices [rows, P] (caller-allocated with cap_rows rows; every cell of the first `rows` rows
 * is written once, zeros included).  Rows are the covering records in record order; row_record[row] int64 = the record.  Cells:
 *   op holding the column   seq                    hap   baseq          mapq
 *   M, =, X                 A,C,G,T -> 1..4 (any case)  tag   qual[query offset]  mapq
 *   D                       -1                     tag   0              mapq
 *   N, or outside [a, b]    0                      0     0              0
 * meta int64 [4] (device) = { rows, status, record, column }: status NSNP_READS_OK, or the first offence in the order the host
 * function meets them (by column, then record): NSNP_READS_TOO_DEEP a column deeper than max_coverage (record -1),
 * NSNP_READS_BAD_HP a covering record whose tag is outside 1..3, NSNP_READS_FOREIGN_BASE a base outside ACGTacgt at a wanted
 * column.  column is the 1-based position.  With a status other than OK the matrices are complete but mean nothing to the
 * reference, which returns nothing then.  The call never aborts on data.
 * The call waits for the stream once, to compare the row count with cap_rows before the outputs are written: NSNP_EINVAL when
 * cap_rows is below it (nothing written), and for null or negative arguments.  NSNP_ESHAPE for R or P above 2^31 - 16. */
#define NSNP_READS_OK 0
#define NSNP_READS_TOO_DEEP 1
#define NSNP_READS_BAD_HP 2
#define NSNP_READS_FOREIGN_BASE 3
size_t nsnp_hap_read_scratch_bytes(int64_t R, int64_t P);
int nsnp_hap_read_depths(nsnp_ctx* ctx, const int64_t* start, const uint32_t* cigar, const int64_t* cigar_off, int64_t R,
                         const int64_t* cols, int64_t P, int32_t* depth, int64_t* rows, void* scratch, void* stream);
int nsnp_hap_read_matrices(nsnp_ctx* ctx, const int64_t* start, const uint8_t* mapq, const int32_t* hp, const uint32_t* cigar,
                           const int64_t* cigar_off, const uint8_t* seq, const uint8_t* qual, const int64_t* seq_off, int64_t R,
                           const int64_t* cols, int64_t P, int64_t max_coverage, int32_t* oseq, int32_t* ohap, int32_t* obq,
                           int32_t* omq, int64_t cap_rows, int64_t* row_record, int64_t* meta, void* scratch, void* stream);

/* ---- stage-4 site groups from the pileup call rows (select_hetesnp_homosnp.py:82-104,180-230) ------------------------------------------
 * Which sites go to the HaplotypeModel, decided from the [N,13] float64 call rows (nsnp_pileup_call_rows: column 0 a position or a key,
 * 1 / 2 the genotype / zygosity argmax, 3 / 4 their maxima) and the reference byte of every row (any case), without the pileup.vcf in
 * between: what merge.select_groups(..., reference_bug=False) finds in the text the row writer (nsnp_vcf_format_batches, batches of
 * batch_size rows restarting with every run) makes of the same rows.  A row is WRITTEN when its argmaxes are below 10 / at most 2, both
 * scores exist and the writer's genotype search does not run off a short batch (nsnp_vcf.c); its genotype text and which score is its QUAL
 * follow the writer.  It is in the DICTIONARY unless its genotype is 0/0 or 1/1 with QUAL >= quality_threshold, a SUPPORT when its
 * genotype is 0/1 with QUAL >= support_quality, a CANDIDATE when QUAL < quality_threshold.  A GROUP is a candidate with adjacent_size
 * supports strictly left and strictly right of it in its own run: 2 adjacent_size + 1 rows in row order.
 *   run_off  device int64 [n_runs + 1], ascending from 0 to N: the rows of every contig, one run each.  Inside a run column 0 must
 *            ascend strictly.
 *   cuts     device float32 [8], merge.group_cuts: the smallest probability whose QUAL reaches quality_threshold, the same for
 *            support_quality (+inf: none does), the first and the last probability that has a score, 1.0 when -0.0 scores as 0.0 does,
 *            three zeros.  The kernels compare bit patterns and evaluate no logarithm.
 *   group_rows int32 / group_keys int64 [cap_groups, 2 adjacent_size + 1] (device): the row index and column 0 of every member, groups in
 *            candidate order.
 *   meta     int64 [4] in device or pinned host memory = { groups found, status, first offending row, supports }.  groups found may
 *            exceed cap_groups: then only the first cap_groups were written.  status NSNP_GROUPS_KEY_ORDER: column 0 of the named row
 *            is not above the row in front of it in the same run (the groups mean nothing then); otherwise the row is -1.
 *   scratch  nsnp_pileup_groups_scratch_bytes(N) bytes of device memory, 16-byte aligned, the caller's (0 = N out of range).  Behind the
 *            call its first N bytes hold the flag byte of every row: NSNP_GROUPS_WRITTEN | _DICT | _CANDIDATE | _SUPPORT | _GROUP (the
 *            candidate of a group) - which contigs have a dictionary entry at all is read from them.
 * The coverage channels are not read: the writer skips a row whose depth is not finite, which counts of reads never are.
 * Asynchronous on `stream`, no host visit.  N == 0 is a no-op that writes meta = 0.  NSNP_EINVAL with nothing launched: N < 0,
 * adjacent_size outside 1..32, batch_size < 1, n_runs < 0 (or 0 with N > 0), cap_groups < 0, a null pointer with N > 0 (group_rows /
 * group_keys may be null with cap_groups 0).  NSNP_ESHAPE for N above 2^31 - 16. */
#define NSNP_GROUPS_OK 0
#define NSNP_GROUPS_KEY_ORDER 1
#define NSNP_GROUPS_WRITTEN   1
#define NSNP_GROUPS_DICT      2
#define NSNP_GROUPS_CANDIDATE 4
#define NSNP_GROUPS_SUPPORT   8
#define NSNP_GROUPS_GROUP     16
size_t nsnp_pileup_groups_scratch_bytes(int64_t N);
int nsnp_pileup_select_groups(nsnp_ctx* ctx, const double* rows, const uint8_t* ref_base, int64_t N, const int64_t* run_off, int n_runs,
                              int64_t batch_size, int adjacent_size, const float* cuts, int32_t* group_rows, int64_t* group_keys,
                              int64_t cap_groups, int64_t* meta, void* scratch, void* stream);

/* host_tensors: the 58 fp32 tensors of model_dev.LSTMNetwork.state_dict() in order
 * (pileup_encoder 26, haplotype_encoder 26, forward_layer 6), HOST pointers.
 * hidden must be a multiple of 64; F = 105 input features; 3 layers as ont_haplotype.yaml. */
int nsnp_hap_load_weights(nsnp_ctx* ctx, const float* const* host_tensors, int n_tensors,
                          int n_features, int hidden, int n_layers, int n_gt, int n_zy);

/* xp: device fp32 [N,105,33], xh: device fp32 [N,105,11] -> gt [N,n_gt], zy [N,n_zy]. */
int nsnp_hap_forward(nsnp_ctx* ctx, const float* xp, const float* xh, int64_t N,
                     float* gt_prob, float* zy_prob, void* stream);

/* ---- scoring a HaplotypeModel checkpoint on labelled sites (HaplotypeModel/evaluate_dev.py:16-86, its eval()) ----------------------------
 * All three arithmetics of the option "hap_precision".  Inference with labels attached: no backward pass.
 *
 * LabelField and EvaluateDataset's target rule (dataset_dev.py:174-187,320) on candidate_labels rows { confident, gt21, zygosity }, device
 * int32 [N,3].  A row is kept when confident == 1 and it is a refcall (zygosity == -1, gt21 < 10) or a variant (0 < zygosity < 10, gt21 < 10);
 * zygosity 0 is in neither list and is dropped, as there.  Of those rows the ones the loaded heads cannot score (gt21 < 0, gt21 >= n_gt,
 * zygosity >= n_zy: where the reference's scatter_ fails) are counted and dropped.  Kept rows, compacted and in their order:
 *   cls   uint8 [N,2]   { gt21, max(zygosity, 0) }          (device)
 *   rows  int64 [N]     the row's index in the pass         (device)
 *   meta  int64 [4]   = { kept, unscorable, refcalls kept, variants kept }; device or pinned host memory
 * Nothing is written behind the kept rows.  Three launches (flags, one-workgroup exclusive scan, compaction), no workgroup waits for another;
 * the scratch is nsnp_pileup_label_classes' (12 bytes per row).  NSNP_ENOWEIGHTS before nsnp_hap_load_weights.  The reference's order -
 * refcalls, then variants, then an unseeded shuffle - is not reproduced: every result that does not depend on the order equals its own. */
int nsnp_hap_label_classes(nsnp_ctx* ctx, const int32_t* label, int64_t N, uint8_t* cls, int64_t* rows, int64_t* meta, void* stream);

/* LSTMNetwork.forward (model_dev.py:120-131) before the two means: the launches of nsnp_hap_forward with a scoring heads kernel as the last.
 * The logit of a head row is computed exactly as nsnp_hap_forward computes it in front of its softmax.  cls uint8 [N,2]: the target classes
 * { gt, zy } (a class outside its head counts as the head's last).  Per site and head h with C classes:
 *   lp = z - logsumexp(z);  site_loss[n,h] = -(0.9 lp[t] + 0.1 / (C - 1) (sum(lp) - lp[t]));  pred[n,h] = first maximum of z
 *   (C == 1: loss 0, pred 0)
 *   counters int64 [n_gt * n_gt + n_zy * n_zy]: two matrices [target][predicted], genotype then zygosity; ADDED to (device memory)
 *   logits   NULL, or fp32 [N, n_gt + n_zy] (genotype rows first): with NULL no logit reaches memory.
 * The heads kernel is persistent: at most NSNP_HAP_EVAL_WAVES_PER_CU waves per compute unit, one site per wave and trip.  Counts are 32-bit
 * integers in LDS, flushed once per workgroup as 64-bit integer adds; no float is added atomically: the same bits from run to run. */
#define NSNP_HAP_EVAL_WAVES_PER_CU 32
int nsnp_hap_eval(nsnp_ctx* ctx, const float* xp, const float* xh, const uint8_t* cls, int64_t N, float* site_loss, uint8_t* pred,
                  int64_t* counters, float* logits, void* stream);

/* nsnp_pileup_batch_loss for rows of two heads: site_loss fp32 [N,2] (8-byte aligned) -> batch_sum double [ceil(N / batch_size), 2]. */
int nsnp_hap_batch_loss(nsnp_ctx* ctx, const float* site_loss, int64_t N, int64_t batch_size, double* batch_sum, void* stream);

/* ---- training the HaplotypeModel: the sample list of a pass under pn_value upsampling (TrainingDataset.__init__, dataset_dev.py:190-230) --
 * cls uint8 [kept,2]: the kept rows' classes as nsnp_hap_label_classes leaves them, device; byte 1 is 0 exactly for a refcall.
 *   samples int64 [cap]  indices in [0, kept) into the kept list (map them through `rows`); the first M are written        (device)
 *   meta    int64 [4]  = { M, refcalls, variants, blocks }; device or pinned host memory
 * The refcalls, in order, are cut into blocks of 1,000; the last holds the remaining 1..1,000.  Block b of len_b refcalls contributes its
 * refcalls in order and then q_b = (int64)((double)len_b * pn_value) variant draws - Python's int(len * pn_value): the float64 product,
 * truncated (int(90 * 0.7) is 62, not 63).  Block b starts at b * (1000 + (int64)(1000.0 * pn_value)): closed form.  M = refcalls + sum q_b.
 * Without a variant every q_b is 0 (the reference's except: branch); without a refcall the list is empty (the reference's quirk too).
 * Draw j of block b picks variant ((uint64)r * variants) >> 32, r = word 0 of Philox4x32-10 at counter { j, b, draw, 0 } under the key
 * { seed & 0xffffffff, seed >> 32 } (csrc/nsnp_philox.hpp).  Multiply-shift departs from uniform by less than variants / 2^32 in total.  The
 * reference draws from an unseeded np.random, so only the distribution is its own; here the list is a pure function of the arguments, the same
 * bits on every run whatever the grid.  `draw` is the caller's pass counter, so that passes differ.  The reference's shuffle inside a block is
 * not made: the caller's permutation of the whole list stands for it and for the DataLoader's.
 * NSNP_EINVAL with nothing written: cap < M, pn_value negative, not finite or above NSNP_HAP_PN_VALUE_MAX (a draw index is 32 bits),
 * kept < 0 or >= 2^32, samples NULL with M > 0.
 * Four launches (refcall flags, the one-workgroup exclusive scan of nsnp_hap_label_classes, the two lists, placement); no workgroup waits for
 * another, nothing is added atomically.  Between the third and the fourth the entry WAITS for the stream once and reads the two counts: cap
 * cannot be held against M without them.  With kept == 0 there is one launch and no wait.  Scratch: nsnp_pileup_label_classes' buffer, 20
 * bytes per kept row (scan, lists, words), grown as there; it is overwritten, so run the entry behind the work that reads a label pass's
 * scratch - on the same stream, or after it has finished. */
#define NSNP_HAP_PN_VALUE_MAX 4194304.0
int nsnp_hap_train_samples(nsnp_ctx* ctx, const uint8_t* cls, int64_t kept, double pn_value, uint64_t seed, uint32_t draw, int64_t* samples,
                           int64_t cap, int64_t* meta, void* stream);

/* ---- training the HaplotypeModel: the loss gradients of a batch (HaplotypeModel/train_dev.py:58-59, model(...) and loss.backward()) ------
 * fp32 only and one device: with hap_precision 1 or 2 nsnp_hap_loss_grad returns NSNP_EINVAL.  The entries need no nsnp_hap_load_weights:
 * the parameters are the caller's device tensors in plain state-dict layout, because they change every step; the packed images of the
 * inference entries are not read and not refreshed (upload a trained state again to score or call with it).
 *
 * nsnp_hap_train_reserve allocates the workspace of the saved activations and gate gradients for chunks of max_sites (1..65,536) sites of a
 * model of n_features (1..128) input features and n_gt, n_zy (each >= 1, at most 16 together) classes; hidden size 256, three layers, windows
 * of 33 and 11 positions.  1,652,864 bytes per site (413,216 floats: gates, c and h of the 222 (layer, direction, step) triples, the masked
 * layer inputs, the gradients) plus 2 MB per 128 (site, step) rows of the pileup window (the weight gradients' slices: 277 MB at 512
 * sites); synchronous.  NSNP_ENOMEM: the previous reservation stays in force.  NSNP_EINVAL for sizes outside these ranges.  A batch larger
 * than the reservation runs in chunks of that size, in order, adding into the same gradients.
 *
 * nsnp_hap_loss_grad, asynchronous on `stream`; every shape follows the dims of the reservation (a caller whose tensors have other dims
 * reserves again first; the Python wrapper refuses them):
 *   params     HOST array of 58 DEVICE pointers, the tensors, order and shapes of nsnp_hap_load_weights
 *   xp, xh     device fp32 [N,F,33] and [N,F,11], as nsnp_hap_eval takes them
 *   cls        device uint8 [N,2] = { genotype, zygosity }; a class outside its head counts as the head's last
 *   keep_masks NULL (no dropout), or a HOST array of 4 device uint8 tensors of 0 / 1: behind pileup layer 0 and pileup layer 1 [N,33,512],
 *              behind haplotype layer 0 and haplotype layer 1 [N,11,512], in the layer output's order [forward 256 | reverse 256].  The next
 *              layer sees h * mask * keep_scale (keep_scale = 1 / (1 - p) of nn.LSTM(dropout=p)), the backward pass applies the same
 *              factor.  NULL gives the bits of all-ones masks with scale 1.
 *   grads      HOST array of 58 device pointers, same shapes: OVERWRITTEN with d(mean gt loss + mean zy loss) / d(param), the means over all
 *              N sites.  bias_ih and bias_hh of a layer and direction receive the same values.
 *   site_loss  NULL, or device fp32 [N,2]: the label-smoothed losses of nsnp_hap_eval
 *   pred       NULL, or device uint8 [N,2]: the first maximum of the genotype / zygosity logits
 * A head of one class has loss 0, pred 0 and gradient 0, as in nsnp_hap_eval.  N == 0 is a no-op (grads untouched).  NSNP_EINVAL for null
 * arguments and without a reservation.  The network runs the reduced schedule of the inference entries (layer 2: 17 of 33 and 6 of 11 steps
 * per direction, dense layer and heads at the centre), which is exact for the gradient too because the loss reads the centre only.  Every
 * matrix product is fp32 MFMA; no floating-point atomics: the same call gives the same bits twice.  nsnp_ctx_read_timing ids 13, 14, 15: the
 * forward, backward and weight-gradient phases of a chunk, one event pair each. */
int nsnp_hap_train_reserve(nsnp_ctx* ctx, int64_t max_sites, int n_features, int n_gt, int n_zy);
int nsnp_hap_loss_grad(nsnp_ctx* ctx, const float* const* params, const float* xp, const float* xh, const uint8_t* cls, int64_t N,
                       const uint8_t* const* keep_masks, float keep_scale, float* const* grads, float* site_loss, uint8_t* pred, void* stream);

/* ---- legacy haplotype caller (HaplotypeModel/predict.py -> model.CatModel; not run by run_caller.sh) ---- */
/* host_tensors: the 132 floating-point tensors of CatModel(nc0=5,nc1=5,nc2=2,nclass=10,nh=256).state_dict()
 * in order, the integer num_batches_tracked entries skipped (6 ResBlocks x 14, haplotype_base.rnn.{0,1} x 10,
 * haplotype_percentage 26, out_layer 2), HOST pointers.  BatchNorm is applied in eval mode (predict.py:28). */
int nsnp_cat_load_weights(nsnp_ctx* ctx, const float* const* host_tensors, int n_tensors);

/* g0, g1: device fp32 [N,40,11,5] exactly as predict.py:33-34,42-43 hands them to the model
 * (g2 / g3 are ignored by CatModel.predict: model.py:332-358) -> gt_prob device fp32 [N,10] (softmax). */
int nsnp_cat_forward(nsnp_ctx* ctx, const float* g0, const float* g1, int64_t N, float* gt_prob, void* stream);

/* Test tap: runs the launches of nsnp_cat_forward (same context options, same kernels, same workspace) up to and including those of
 * `stage`, then ONE un-tiling launch that writes that stage's image to `out` as plain fp32 in natural order - only the used channels
 * and features, the unit_of_pos storage order of an LSTM's h undone, an f16x3 (hi, lo) pair decoded as hi + lo - and returns.
 * One pass only: 0 < N <= 4096.  out_floats must be the stage's size exactly.  NSNP_EINVAL otherwise, nothing launched.
 *   stage                         image                                   out
 *   NSNP_CAT_ST_PIXELS            torch.cat((g0, g1), 1) as channels      [N,10,40,11]
 *   NSNP_CAT_ST_BLOCK_Y + 2 i     ResBlock i: relu(bn1(conv1 x))          [N,C,H,W], C = 32,64,128,128,256,256, H = 40,20,10,10,3,3
 *   NSNP_CAT_ST_BLOCK_OUT + 2 i   ResBlock i: relu(bn2(conv2 y) + sc(x))  the same
 *   NSNP_CAT_ST_POOL + k          the max-pool after block 0, 1, 3        [N,32,20,11], [N,64,10,11], [N,128,3,11]
 *   NSNP_CAT_ST_SEQ0              the last pool = the LSTM's input        [11,N,256]
 *   NSNP_CAT_ST_PCT_FEATURES      calculate_percentage                    [11,N,20]
 *   NSNP_CAT_ST_PCT_H + l         h of percentage layer l = 0, 1          [11,N,512] = [h_fwd ; h_bwd]
 *                    + 2          the third layer runs six steps per direction: row s = [h_fwd(column s) ; h_bwd(column 10 - s)]   [6,N,512]
 *   NSNP_CAT_ST_PCT_LINEAR        haplotype_percentage.out_layer at column 5   [N,256]
 *   NSNP_CAT_ST_RNN0_H            h of haplotype_base.rnn.0               [11,N,512]
 *   NSNP_CAT_ST_RNN0_EMB          its embedding                           [11,N,256]
 *   NSNP_CAT_ST_RNN1_H            h of haplotype_base.rnn.1, six steps as above (row 5 = column 5)   [6,N,512]
 *   NSNP_CAT_ST_CAT               the 512-vector in front of out_layer    [N,512]
 * Later stages overwrite the buffers of earlier ones, which is why a stage is read by a run that stops there. */
#define NSNP_CAT_ST_PIXELS        0
#define NSNP_CAT_ST_BLOCK_Y       1
#define NSNP_CAT_ST_BLOCK_OUT     2
#define NSNP_CAT_ST_POOL          13
#define NSNP_CAT_ST_SEQ0          16
#define NSNP_CAT_ST_PCT_FEATURES  17
#define NSNP_CAT_ST_PCT_H         18
#define NSNP_CAT_ST_PCT_LINEAR    21
#define NSNP_CAT_ST_RNN0_H        22
#define NSNP_CAT_ST_RNN0_EMB      23
#define NSNP_CAT_ST_RNN1_H        24
#define NSNP_CAT_ST_CAT           25
#define NSNP_CAT_N_STAGES         26
int nsnp_cat_forward_stage(nsnp_ctx* ctx, const float* g0, const float* g1, int64_t N, int stage, float* out, int64_t out_floats, void* stream);

/* Builds one group tensor [N,40,length,5] fp32 from the per-tag matrices the HDF5 bins hold
 * (dataset.py:862-915): read / base-quality / mapping-quality [N,depth,length] int32 per tag; the first 20
 * rows of tag 1 then of tag 2; planes (base, baseq, mapq, mask = base != -2, phase = 1 | 2).
 * depth1, depth2 >= 20 (NSNP_ESHAPE otherwise: the reference's [:20] slicing would yield a ragged tensor). */
int nsnp_cat_groups(nsnp_ctx* ctx, const int32_t* read1, const int32_t* bq1, const int32_t* mq1, int depth1,
                    const int32_t* read2, const int32_t* bq2, const int32_t* mq2, int depth2,
                    int64_t N, int length, float* g, void* stream);

/* ---- result gather over RCCL (optional; see the note at the top) ---------------------------------------- */
/* Rank 0 obtains 128 opaque bytes and shares them with the other ranks by any side channel; every rank then binds a
 * communicator to its context (collective call).  NSNP_ENOTSUP when no RCCL library can be resolved. */
int nsnp_comm_unique_id(uint8_t* id128);
int nsnp_comm_init(nsnp_ctx* ctx, const uint8_t* id128, int rank, int world);
/* A host that already owns a communicator (nsnp_gather_results(ctx, rccl_comm, ...)) binds it instead:
 * rccl_comm is its ncclComm_t, rank / world as it was created.  The context borrows it: nsnp_comm_destroy and
 * nsnp_ctx_destroy only forget it.  The communicator must come from the RCCL image this library resolves (the one already
 * loaded in the process). */
int nsnp_comm_attach(nsnp_ctx* ctx, void* rccl_comm, int rank, int world);
int nsnp_comm_destroy(nsnp_ctx* ctx);
/* Rooted gather of per-rank byte blocks (device memory) into root_buf (device, root only) at byte_off[r] .. byte_off[r+1].
 * byte_off is a HOST array of world + 1 offsets and is required on EVERY rank (byte_off[0] == 0, non-decreasing,
 * byte_off[rank + 1] - byte_off[rank] == local_bytes): all ranks validate the same table before anything is posted, so a bad
 * plan fails everywhere with NSNP_EINVAL instead of leaving peers in an unmatched send.  Grouped ncclSend / ncclRecv on
 * `stream`, asynchronous; rank order = site order, so the merge is a concatenation.  nsnp_gather_check is the device-free
 * part of that validation (usable to pre-check a plan). */
int nsnp_gather_check(int rank, int world, int64_t local_bytes, const int64_t* byte_off, int root);
int nsnp_gather_results(nsnp_ctx* ctx, const void* local, int64_t local_bytes, void* root_buf,
                        const int64_t* byte_off, int root, void* stream);

#ifdef __cplusplus
}
#endif
#endif
