/*
 * gym_amd.h — C ABI of the MI355X (gfx950) strategy-communication-step kernels.
 *
 * This is the drop-in boundary under EXO Gym's Strategy API (reference:
 * satoutahhaithem/gym @ 2025-07-11).  Every entry point replaces the per-tensor
 * torch op loop of one reference function; the replaced interface is cited on
 * each declaration as `file:line` relative to the reference root.
 *
 * Conventions:
 *   - plain pointers + element counts; no torch types cross this boundary;
 *   - the caller (PyTorch) owns every buffer: the library never allocates or
 *     frees device memory and keeps no mutable global state other than a
 *     thread-local error string;
 *   - all work is enqueued asynchronously on the given hipStream_t (pass the
 *     torch current stream); nothing synchronises the host;
 *   - every function returns 0 on success or a GA_E* code; the message for the
 *     last failure on the calling thread is available from ga_last_error().
 *
 * A "replica set" is K simulated-node copies of one flat parameter arena laid
 * out as [K, ld] (replica k starts at element k*ld).  K = 1 is the ordinary
 * one-node-per-GPU case; K > 1 is batched-replica mode.
 */
#ifndef GYM_AMD_H
#define GYM_AMD_H

#include <stdint.h>
#include <hip/hip_runtime_api.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GA_API __attribute__((visibility("default")))

/* error codes */
#define GA_OK 0
#define GA_EINVAL 1   /* bad argument (null pointer, bad size, unknown dtype) */
#define GA_EHIP 2     /* a HIP runtime call or kernel launch failed */
#define GA_EUNSUP 3   /* unsupported configuration */

/* element types of arena buffers */
#define GA_F32 0
#define GA_BF16 1
/* DeMo only (ga_demo_encode / ga_demo_decode): bf16 arenas with the reference's
 * bf16 arithmetic -- bf16 DCT bases (the caller's F / B tables hold
 * bf16-representable values), every stage of each transform rounded to bf16 in
 * the reference's contraction order (chunk rows first), the delta rounded after
 * the decay and after the gradient add (exogym/strategy/demo_impl/demo.py:
 * 159-180, 235-252 as torch runs it); the decode's scatter-mean adds the sources
 * in node order with the sum rounded to bf16 after every add, then divides
 * (demo.py:339-341: torch's bf16 scatter_reduce; on the GPU its atomic adds run
 * in an unspecified order, so at 3+ hitters of one position node order is one
 * of the orders the reference can produce). */
#define GA_BF16_REF 2

/* replica-set layouts (SPARTA entry points):
 *   GA_LAYOUT_ROWS        [K, ld]: replica k of element i at k*ld + i (every other kernel's layout)
 *   GA_LAYOUT_ELEM_MAJOR  [n, ld]: replica k of element i at i*ld + k (ld >= K): the K replicas of
 *                         one element are adjacent, so a sparse gather moves whole lines */
#define GA_LAYOUT_ROWS 0
#define GA_LAYOUT_ELEM_MAJOR 1

/* SPARTA mask formats:
 *   GA_MASK_BYTES  uint8 per element (selected iff != 0), 16-byte aligned
 *   GA_MASK_BITS   uint64 words, bit j of word w = element 64 w + j (ga_sparta_pack_mask) */
#define GA_MASK_BYTES 0
#define GA_MASK_BITS 1
#define GA_MASK_TORCH 2

/* GA_MASK_TORCH: the mask argument points to this HOST struct, and the select /
 * average kernels draw the reference's masks themselves, exactly as
 * ga_sparta_torch_bernoulli would write them (no mask in memory). */
typedef struct ga_sparta_torch_draw {
    const int64_t* table;     /* device rows {arena offset (multiple of 64), numel, -} per drawn tensor, ascending */
    int32_t ntens;            /* rows */
    float p;                  /* selection probability as torch.full(shape, p) holds it (fp32) */
    uint64_t seed, offset0;   /* torch generator state for the first drawn tensor */
    uint64_t offset_step;     /* generator offset per tensor (12) */
    const uint64_t* seedoff;  /* device {seed, offset0} overriding the two above, or null */
} ga_sparta_torch_draw;

/* ---- library ---------------------------------------------------------- */

/* ABI version (major*100 + minor). */
GA_API int ga_abi_version(void);

/* Message describing the last failure on the calling thread ("" if none). */
GA_API const char* ga_last_error(void);

/*
 * Calibration helper (no reference counterpart): dst <- src, nbytes (a multiple
 * of 16, 16-byte aligned buffers) as a float4 streaming copy.  bench.py times
 * it in the same process as the step kernels, so a roofline fraction can be
 * read against what the box actually streams.
 */
GA_API int ga_stream_copy(const void* src, void* dst, int64_t nbytes, hipStream_t stream);

/*
 * Calibration helper (no reference counterpart): the random-word floor of the
 * [K, ld] rows layout.  For each of the M positions pos[j] (int32, ascending)
 * and each replica k < K, the fp32 word at a[k * ld + pos[j]] is read and
 * (write != 0) written back as x * 0.5 + 1, one lane per (position, replica),
 * replica-major within 16384-element tiles as the SPARTA rows kernel walks
 * them -- the same 4-B words at random 64-B sectors, without the mask.  bench.py
 * times it on the positions a SPARTA step selected, in the same process.
 * write = 2 / 3: the whole aligned 64-B sector / 128-B line holding the word is
 * read and written back instead (ld a multiple of 32, a 128-B aligned): what a
 * full-sector write-back would cost against the word's partial write.
 */
GA_API int ga_probe_random_words(float* a, int64_t ld, int64_t K, const int32_t* pos, int64_t M, int write,
                                 hipStream_t stream);

/*
 * Calibration helper (no reference counterpart): the Philox4x32-10 issue
 * ceiling of the reference's SPARTA mask draw (sparta.py:80-85 through
 * ga_sparta_torch_bernoulli).  The n / 4 calls an n-element draw makes, in
 * ga_sparta_torch_bernoulli's packed-word launch shape (one lane per 64
 * elements, four independent chains), with the words XOR-folded instead of
 * compared and packed and nothing stored (sink: one device uint32, written only
 * in the never-taken case).  bench.py times it to give the draw a VALU roofline.
 */
GA_API int ga_probe_philox(int64_t n, uint32_t* sink, hipStream_t stream);

/*
 * Calibration helper (no reference counterpart): the memory floor of the DeMo
 * codec's access pattern (demo_impl/demo.py:142-209 through ga_demo_encode_sym /
 * ga_demo_decode_sym).  One wavefront per 64x64 chunk of a [rows, cols] fp32
 * matrix (rows, cols multiples of 64), the chunk kernels' grid and coalesced
 * layout, no transform: mode 0 reads a and b and writes a (the encode's 12 B per
 * element), mode 1 reads a and writes a and b (the decode's).  bench.py prices
 * the codec kernels against it on a matrix of the model's size.
 */
GA_API int ga_probe_chunk_stream(float* a, float* b, int64_t rows, int64_t cols, int mode, hipStream_t stream);

/*
 * Placement probe (no reference counterpart) for the fused DiLoCo outer step:
 * ga_diloco_outer's access pattern over an fp32 [K, ld_src] replica set (K <= 16)
 * and a master / momentum pair -- every stream read and written back through the
 * kernel's own loads and stores -- with every value unchanged.  On MI355X the
 * step's rate depends on where master / momentum sit physically relative to the
 * replicas (1.65 vs 1.88 ms at GPT-2 124M x 8 for the same virtual layout,
 * profiles/r04b_placement_search_p*.txt); DiLoCoOuter times candidate buffers with
 * this probe once and keeps the fastest (gym_amd/engine.py).
 */
GA_API int ga_probe_diloco_placement(float* src, int64_t K, int64_t ld_src, int64_t n, float* master, float* mom,
                                     hipStream_t stream);

/*
 * Placement probe (no reference counterpart) for the in-place replica mean
 * (ga_replica_mean with dst == src, the SimpleReduce / FedAvg step over K local
 * replicas): its access pattern over an fp32 [K, ld_src] set (K <= 16, n a
 * multiple of 4) with every value written back unchanged.  The in-place mean over
 * GPT-2 124M x 8 runs 1.49 ms in an ordinary allocation and 1.26 ms in the
 * fastest of 12 fresh ones (profiles/r05y_mean_placement.txt); MeanReduce times
 * candidate sets with this probe once and moves the caller's set to the fastest.
 */
GA_API int ga_probe_mean_placement(float* src, int64_t K, int64_t ld_src, int64_t n, hipStream_t stream);

/*
 * Placement probe (no reference counterpart) for the fused Adam/AdamW step:
 * ga_adam_step's access pattern over fp32 [K, ld] param / grad / exp_avg /
 * exp_avg_sq sets (n a multiple of 4, 16-byte aligned) -- p, g, m, v read, p, m,
 * v written back unchanged.  ArenaAdam times candidate physical buffers for the
 * moments with it once (the step ran 0.553-0.625 ms at GPT-2 124M by where they
 * sit, profiles/r04k_adam_placement.txt).
 */
GA_API int ga_probe_adam_placement(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t K,
                                   int64_t ld, int64_t n, hipStream_t stream);

/* ---- mean reduce: SimpleReduce / FedAvg / DiLoCo averaging ------------- */

/*
 * dst_j[i] = (sum_{k<K} src[k*ld_src + i]) / divisor   for j < K_out, i < n
 * (dst_j = dst + j*ld_dst).  Sum in ascending k, fp32 accumulation, then a
 * correctly rounded true division (reference quirk Q2: division, not *1/K).
 * If `rows` is non-null it is a device array of K int32 replica indices and
 * replica rows[k] is read instead of replica k (FedAvg islands).
 * dst may alias src (in-place all-replica average).  divisor == 1 gives a sum.
 *
 * Replaces: exogym/strategy/strategy.py:130-133 (per-param all_reduce + div_),
 *           exogym/strategy/diloco.py:34-37, exogym/strategy/federated_averaging.py:53-69,
 *           exogym/trainer.py:95-119 (final state averaging).
 */
GA_API int ga_replica_mean(int dtype, const void* src, int64_t K, int64_t ld_src,
                           const int32_t* rows, int64_t n, float divisor,
                           void* dst, int64_t K_out, int64_t ld_dst, hipStream_t stream);

/* ---- DiLoCo outer step -------------------------------------------------- */

/*
 * Fused DiLoCo outer step over n elements (one arena or one shard of it):
 *   avg  = (sum_{k<K} src_k[i]) / divisor                 (diloco.py:34-37)
 *   g    = master[i] - avg                                (diloco.py:43-45)
 *   g   += weight_decay * master[i]          if weight_decay != 0
 *   buf  = first_step ? g : momentum*buf + (1-dampening)*g   if momentum != 0
 *   g    = nesterov ? g + momentum*buf : buf                  if momentum != 0
 *   master[i] -= lr * g                                   (torch SGD, diloco.py:70)
 *   dst_j[i] = master[i]  for j < K_out                   (diloco.py:47-49 + 39-41)
 * `mom` may be null when momentum == 0.  master and mom are fp32 when
 * master_f32 != 0, otherwise they share `dtype` with src/dst.
 *
 * Replaces: exogym/strategy/diloco.py:51-76 (the outer-step branch) and the
 * CPU torch.optim.SGD it drives (diloco.py:26-28,86).
 */
GA_API int ga_diloco_outer(int dtype, const void* src, int64_t K, int64_t ld_src,
                           int64_t n, float divisor, void* master, void* mom,
                           int master_f32, int first_step, float lr, float momentum,
                           float dampening, float weight_decay, int nesterov,
                           void* dst, int64_t K_out, int64_t ld_dst, hipStream_t stream);

/*
 * SPARTA's sparse average and the outer step that follows it on a DiLoCo
 * boundary step (SPARTA+DiLoCo: sparta_diloco.py), as the outer step's one pass.
 * `bits` are the packed mask words of ga_sparta_pack_mask / ga_sparta_torch_bernoulli
 * (GA_MASK_BITS), ceil(n / 64) of them.  An element whose bit is clear is
 * ga_diloco_outer's; a selected one takes the arithmetic of
 * ga_sparta_average_local followed by ga_diloco_outer:
 *   s  = sum_{k<K} src_k[i]                      (fp32, ascending k)
 *   a  = s / sparse_divisor, rounded to `dtype`  (what SPARTA stores in every row)
 *   s' = a + a + ... (K fp32 additions from 0)   (what the outer step then sums)
 * and the update above on s'.  Bit-identical to the two launches.  Valid only
 * where the outer step overwrites every row the average wrote: dst == src,
 * K_out == K, ld_dst == ld_src, else GA_EINVAL.  master and mom are fp32
 * (master_f32 != 0 for a bf16 set).  Algorithmic bytes (2K + 4) * 4 n + n / 8
 * for fp32.
 */
GA_API int ga_diloco_outer_masked(int dtype, void* src, int64_t K, int64_t ld_src, int64_t n,
                                  const uint64_t* bits, float sparse_divisor, float divisor,
                                  void* master, void* mom, int master_f32, int first_step,
                                  float lr, float momentum, float dampening, float weight_decay,
                                  int nesterov, void* dst, int64_t K_out, int64_t ld_dst,
                                  hipStream_t stream);

/*
 * The outer step with an Adam / AdamW outer optimizer (OptimSpec "adam" / "adamw" as
 * DiLoCo's outer_optim_spec, diloco.py:26-28), one pass over n elements:
 *   avg = (sum_{k<K} src_k[i]) / divisor         (fp32, ascending k, true division)
 *   g   = master[i] - avg
 *   ga_adam_step's element update of (master[i], g, exp_avg[i], exp_avg_sq[i]) with
 *   the eight scalars below (torch's _multi_tensor_adam order; see ga_adam_step)
 *   dst_j[i] = master[i]  for j < K_out
 * master, exp_avg and exp_avg_sq are fp32 whatever `dtype` (f32 / bf16 src and dst).
 * There is no first-step flag: zero moments and the bias corrections of step 1
 * (step_size = -lr / (1 - beta1), bc2_sqrt = sqrt(1 - beta2)) give torch's first
 * step.  Argument checks as ga_diloco_outer.  Algorithmic bytes (2K + 6) * 4 n for
 * fp32, in place over K rows.
 */
GA_API int ga_diloco_outer_adam(int dtype, const void* src, int64_t K, int64_t ld_src, int64_t n,
                                float divisor, float* master, float* exp_avg, float* exp_avg_sq,
                                float lerp_w, float beta2, float one_m_beta2, float eps, float wd_factor,
                                float l2_wd, float step_size, float bc2_sqrt, void* dst, int64_t K_out,
                                int64_t ld_dst, hipStream_t stream);

/*
 * ga_diloco_outer_masked with the Adam update of ga_diloco_outer_adam: SPARTA's
 * sparse average over the elements selected in `bits` and the outer step, one
 * pass, bit-identical to ga_sparta_average_local followed by ga_diloco_outer_adam.
 * In place over all K rows only (dst == src, K_out == K, ld_dst == ld_src).
 */
GA_API int ga_diloco_outer_adam_masked(int dtype, void* src, int64_t K, int64_t ld_src, int64_t n,
                                       const uint64_t* bits, float sparse_divisor, float divisor,
                                       float* master, float* exp_avg, float* exp_avg_sq, float lerp_w,
                                       float beta2, float one_m_beta2, float eps, float wd_factor,
                                       float l2_wd, float step_size, float bc2_sqrt, void* dst,
                                       int64_t K_out, int64_t ld_dst, hipStream_t stream);

/*
 * The delayed, mixed merge of the streaming outer step (Streaming DiLoCo): the SGD /
 * Nesterov outer update on a staged sum (or on the live rows), then every live row
 * blended with the new master instead of overwritten.  Per element i, every line one
 * individually rounded fp32 operation:
 *   sum = 0.f + src_0[i] + ... + src_{K-1}[i]            (ascending k)
 *   m   = ga_diloco_outer's update of (sum, master[i], mom[i]): avg = sum / divisor,
 *         g = master[i] - avg, and its lines from there on, with the same fmaf's
 *   master[i] = m;  mom[i] = buf                          (momentum != 0)
 *   alpha == 0:  x_j[i] = T(m)                            x is not read
 *   otherwise:   x_j[i] = T(fmaf(alpha, float(x_j[i]), (1.f - alpha) * m))   for j < K_out
 * T is `dtype` (GA_F32 / GA_BF16, of src and x); master and mom are fp32, mom may be
 * null when momentum == 0.  K_out may be 0 (state update only).  x may alias src when
 * it is the same set (same base, K_out == K, ld_x == ld_src: the in-place one-process
 * step): every source of an element is read before any store to it, and x_j[i] is read
 * before it is written and never after.  alpha outside [0, 1) is GA_EINVAL; the other
 * argument checks are ga_diloco_outer's.  With alpha == 0 the result is bit-identical to
 * ga_diloco_outer with an fp32 master.  Algorithmic bytes per element (fp32): 4 K + 16
 * (8 without momentum) + 4 K_out, or 8 K_out when alpha != 0.
 */
GA_API int ga_diloco_outer_merge(int dtype, const void* src, int64_t K, int64_t ld_src, int64_t n, float divisor,
                                 float* master, float* mom, int first_step, float lr, float momentum,
                                 float dampening, float weight_decay, int nesterov, float alpha,
                                 void* x, int64_t K_out, int64_t ld_x, hipStream_t stream);

/*
 * The island outer step (no reference counterpart: the reference's outer step averages
 * the world, diloco.py:34-37): every node takes ga_diloco_outer's SGD / Nesterov update
 * against the average of its island, on a master and a momentum row of its own, all
 * islands in one pass.  src holds S rows of `dtype` (GA_F32 / GA_BF16).  starts,
 * members and slots are DEVICE int32 arrays: starts[0..I] delimits island j's entries
 * in members and slots; members[e] is a source row in [0, S), ascending within an
 * island; slots[e] is the row in [0, K_state) of that member's master, momentum and x,
 * or -1 for a member hosted elsewhere, which is summed and not updated.  For island j
 * with entries e0 = starts[j] .. e1 = starts[j + 1], per element i, every line one
 * individually rounded fp32 operation:
 *   sum = 0.f + src_{members[e0]}[i] + ... + src_{members[e1-1]}[i]     (ascending e)
 *   for every entry e with slot = slots[e] >= 0:
 *     m = ga_diloco_outer's update of (sum, divisor = float(e1 - e0), master_slot[i],
 *         mom_slot[i]): avg = sum / divisor, g = master_slot[i] - avg, and its lines
 *         from there on (weight decay, first step, momentum, dampening, Nesterov,
 *         master -= lr * g), with the same fmaf's
 *     master_slot[i] = m;  mom_slot[i] = buf                (momentum != 0)
 *     x_slot[i] = T(m)
 * master and mom are fp32 [K_state, ld_state], mom may be null when momentum == 0; x is
 * [K_state, ld_x] of `dtype`.  first_step is one flag for the launch.  Rows of master,
 * mom and x that no slot names are not touched, nor is anything past n in a row.
 * The caller's contract, which the host cannot check on device tables and the kernel
 * does not: every index is in range, every slot appears at most once, no island is
 * empty.  x may alias src (the in-place step, slot == member row): a thread reads every
 * member of its (island, vector) before it stores any, the stores of a vector go to
 * rows of that island only, and no two threads share a vector of a row.  The vector
 * path (16 B per lane, 8 B for bf16) runs when n % 4 == 0, the bases are so aligned and
 * the lds are multiples of 4; otherwise an element path runs the same arithmetic.
 * GA_EINVAL: n < 0, S < 1, K_state < 1, I < 1 or I > 65535 (the island is a grid
 * dimension); a null src, master, x or table, or a null mom with momentum != 0; ld_src
 * < n with S > 1; ld_x or ld_state < n with K_state > 1; master or mom not 4-byte
 * aligned; Nesterov without a momentum or with dampening; an unknown dtype.  n == 0 is
 * a no-op.  Algorithmic bytes per element of an island of s members of which L are
 * local, fp32: 4 s + (16 + 4) L, or (8 + 4) L without momentum; with every member
 * local that is 24 per node and element.
 */
GA_API int ga_diloco_outer_islands(int dtype, const void* src, int64_t S, int64_t ld_src, int64_t n,
                                   const int32_t* starts, int64_t I, const int32_t* members,
                                   const int32_t* slots, float* master, float* mom, int64_t K_state,
                                   int64_t ld_state, int first_step, float lr, float momentum,
                                   float dampening, float weight_decay, int nesterov, void* x, int64_t ld_x,
                                   hipStream_t stream);

/* ---- DiLoCo outer step on int8 / int4 block-quantised pseudo-gradients --- */

/*
 * The quantised format, on the wire and in memory (no reference counterpart: the
 * reference's outer step all-reduces fp32, diloco.py:34-37).  Blocks are 256
 * consecutive elements of an arena row, nb = ceil(n / 256), the last may be short;
 * bits is 8 or 4, qmax 127 or 7.  One payload row per node, in bytes:
 *   [ q : nb * 256 * bits / 8 ][ scales : nb x fp32 ]
 * int8: one two's-complement byte per element; int4: byte j of a block holds
 * element 2j in bits 0-3 and element 2j + 1 in bits 4-7 (two's-complement nibbles).
 * Elements past n in the last block and the pad bytes are 0.
 * ga_quant_row_bytes: that size rounded up to a multiple of 16 (host only; -1 for
 * n < 0 or bits outside {4, 8}).
 */
GA_API int64_t ga_quant_row_bytes(int64_t n, int bits);

/*
 * Encode the pseudo-gradients of K rows x [K, ld_x] (f32 / bf16) against an fp32
 * master into K payload rows (row k at payload + k * ld_q_bytes).  Every line is one
 * individually rounded fp32 operation:
 *   d    = master[i] - float(x[k, i])
 *   d    = d + residual[k, i]                  (residual != null: error feedback)
 *   amax = max over the block of |d|
 *   !(amax >= 2^-100):  s = 0 and every q of the block = 0
 *   else  s = amax / qmax, inv = qmax / amax   (IEEE fp32 divisions)
 *         q = clamp((int)rintf(d * inv), -qmax, qmax)
 *   scales[k, b] = s
 *   residual[k, i] = d - float(q) * s          (residual != null; mul, then sub)
 * residual is an fp32 [K, ld_r] set or null.  ld_q_bytes >= ga_quant_row_bytes(n,
 * bits) and a multiple of 16, payload 16-byte aligned; bytes of a payload row past
 * its row_bytes are not written.  x / master / residual may have any element
 * alignment and ld (16-byte vector access when aligned, element access otherwise,
 * the same bytes either way).  Only finite inputs are in contract: a non-finite
 * value does not fault, its block's result is unspecified.
 */
GA_API int ga_quant_encode(int dtype, const void* x, int64_t K, int64_t ld_x, const float* master,
                           float* residual, int64_t ld_r, int64_t n, int bits, void* payload,
                           int64_t ld_q_bytes, hipStream_t stream);

/*
 * Decode S payload rows (ga_quant_encode's format, row r at payload + r *
 * ld_q_bytes, node order) and take the outer step, one pass over n elements:
 *   acc = 0; for r in 0..S-1: acc = acc + float(q_r[i]) * s_r[block of i]
 *   g   = acc / divisor
 *   ga_diloco_outer's update from its pseudo-gradient on (weight decay, first step,
 *   momentum, dampening, Nesterov, master -= lr * g) on the fp32 master / mom
 *   dst_j[i] = master[i] rounded to `dtype`  for j < K_out
 * S has no upper limit.  mom may be null when momentum == 0.  Algorithmic bytes per
 * element: S * (bits / 8 + 1 / 64) + 16 (8 without momentum) + K_out * sizeof(dtype).
 */
GA_API int ga_diloco_outer_dequant(const void* payload, int64_t S, int64_t ld_q_bytes, int bits, int64_t n,
                                   float divisor, float* master, float* mom, int first_step, float lr,
                                   float momentum, float dampening, float weight_decay, int nesterov, int dtype,
                                   void* dst, int64_t K_out, int64_t ld_dst, hipStream_t stream);

/* ---- SPARTA sparse averaging ------------------------------------------- */

/* Workspace bytes needed by ga_sparta_select for an arena of n elements. */
GA_API int64_t ga_sparta_workspace_bytes(int64_t n);

/*
 * Gap table of the Philox mask stream for selection rate p (64 entries):
 * table[j] = round(2^32 * (1 - (1 - p)^(j + 1))) (0 for p <= 0, 2^32 for
 * p >= 1), nondecreasing.  Each 64-element group g of the arena reads the
 * 32-bit words of philox4x32_10(key = seed, ctr = {g, r, iteration_lo,
 * iteration_hi}), r = 0, 1, ..., in order (x, y, z, w); starting at pos = 0,
 * a word u >= table[63] ends the group, otherwise pos += #{j : table[j] <= u},
 * element 64 g + pos is selected if pos < 64, and pos += 1 (the group ends at
 * pos >= 64).  The gaps are Geometric(p): every element is selected
 * independently with probability p (up to the 2^-32 rounding of the table).
 */
GA_API void ga_sparta_gap_table(double p, uint64_t* table);

/*
 * bits[w] = OR_j (mask[64 w + j] != 0) << j over the n-element uint8 mask
 * arena, ceil(n/64) words, bits past n zero: rank 0's selector masks in the
 * form they are broadcast at N > 1 (n/8 bytes on the wire instead of the
 * reference's n bool bytes per step, sparta.py:32-37).
 */
GA_API int ga_sparta_pack_mask(const uint8_t* mask, int64_t n, uint64_t* bits, hipStream_t stream);

/*
 * The reference's per-tensor mask draw, RandomIndexSelector.get_indices =
 * torch.bernoulli(torch.full(shape, p, device=cuda)) (sparta.py:80-85), for
 * every drawn tensor in one launch, bit-identical to ATen's HIP kernel for it:
 * tensor i (table row i = {arena offset (a multiple of 64), numel, first
 * workgroup}, each workgroup ga_sparta_torch_bernoulli_span() elements of one
 * tensor, nblocks in total) uses generator offset offset0 + i * offset_step; element
 * 4t + j of the tensor is selected iff the j-th uniform of Philox4x32-10
 * (key seed, counter {offset/4, t}) is <= p.  GA_MASK_BYTES: mask[offset + e]
 * <- 0/1; GA_MASK_BITS (arena offsets multiples of 64): the tensor's bits of
 * the packed words (ga_sparta_pack_mask layout; words of tensors not drawn
 * are left as they are).  If seedoff != null (device memory, {seed,
 * offset0}) those replace the seed/offset0 arguments: the generator state rank
 * 0 broadcast (16 bytes), so every rank draws rank 0's masks (the reference
 * broadcasts the masks themselves, sparta.py:32-37).  The caller advances its
 * torch generator by ntens * offset_step.
 */
/* sizeof(ga_sparta_torch_draw) (binding layout check). */
GA_API int ga_sparta_torch_draw_bytes(void);

/* Elements per workgroup of ga_sparta_torch_bernoulli (the table's first-workgroup unit). */
GA_API int64_t ga_sparta_torch_bernoulli_span(void);

GA_API int ga_sparta_torch_bernoulli(const int64_t* table, int32_t ntens, int64_t nblocks, float p,
                                     uint64_t seed, uint64_t offset0, uint64_t offset_step,
                                     const uint64_t* seedoff, void* mask, int mask_format,
                                     hipStream_t stream);

/*
 * Select the SPARTA index set over an arena of n elements and gather the
 * selected values summed over the K local replicas (replica set in `layout`,
 * GA_LAYOUT_*).
 *   mask source: if mask != null, element i is selected iff its mask entry is
 *   set (mask_format GA_MASK_BYTES: uint8 mask arena, GA_MASK_BITS: the packed
 *   words of ga_sparta_pack_mask -- rank 0's per-tensor index_selector masks,
 *   broadcast, sparta.py:32-37; GA_MASK_TORCH: mask -> a host
 *   ga_sparta_torch_draw, the reference's draw computed in-kernel); otherwise
 *   the in-kernel Philox4x32-10 stream decides
 *   with selection rate p (see ga_sparta_gap_table), except inside the `nskip` element ranges skip[2r] <= i < skip[2r+1]
 *   (sorted, disjoint: the tensors without a gradient, which the reference
 *   skips, sparta.py:29-30; skip may be null when nskip == 0).
 * Outputs (device): idx[j] = j-th selected element index in ascending order
 * (row-major over the arena, == param.data[mask] order, sparta.py:38),
 * vals[j] = sum_k src_k[idx[j]], count[0] = number selected (int64),
 * count[1] = 1 if that exceeded `cap` (only the first cap are written).
 * `work` must hold ga_sparta_workspace_bytes(n) bytes.
 * The sum is accumulated in fp32 in ascending replica order; with a bf16 set
 * vals[j] holds that fp32 sum rounded once to bf16 (nearest even), and
 * ga_sparta_scatter divides the rounded value.
 *
 * Replaces: RandomIndexSelector.get_indices (sparta.py:80-85), the mask
 * broadcast and gather of SparseCommunicator.communicate (sparta.py:24-38).
 */
GA_API int ga_sparta_select(int dtype, const void* src, int64_t K, int64_t ld,
                            int layout, int64_t n, const void* mask, int mask_format,
                            uint64_t seed, uint64_t iteration, double p,
                            const int64_t* skip, int64_t nskip, int64_t cap,
                            int32_t* idx, void* vals, int64_t* count, void* work,
                            hipStream_t stream);

/*
 * dst_k[idx[j]] = vals[j] / divisor for j < min(count[0], cap), k < K
 * (replica set in `layout`, GA_LAYOUT_*): a true fp32 division, rounded to the
 * set's dtype.  With a bf16 set vals[j] is the bf16 that ga_sparta_select stored
 * (the fp32 sum rounded once), so the select -> scatter path rounds twice where
 * ga_sparta_average_local rounds once.
 * Replaces: `sparse_data /= num_nodes; param.masked_scatter_(mask, sparse_data)`
 * (sparta.py:40-42).
 */
GA_API int ga_sparta_scatter(int dtype, const void* vals, const int32_t* idx,
                             const int64_t* count, int64_t cap, float divisor,
                             void* dst, int64_t K, int64_t ld, int layout, hipStream_t stream);

/*
 * Single-process SPARTA step (every node is a local replica, no exchange):
 * select as ga_sparta_select, then each selected element of every replica
 * <- (sum over the K replicas) / divisor, in the same pass (the gathered lines
 * are written back while still in L2).  idx/vals/count/work may all be null
 * (no packed list, no count/scan pass); if given they are filled as by
 * ga_sparta_select.  Any positive divisor (not only the replica count, not only
 * powers of two) gives the correctly rounded quotient of the fp32 sum
 * (ascending replica order), subnormal quotients included, rounded once to the
 * set's dtype.  Replaces sparta.py:24-44 for batched replicas.
 */
GA_API int ga_sparta_average_local(int dtype, void* reps, int64_t K, int64_t ld, int layout, int64_t n,
                                   const void* mask, int mask_format, uint64_t seed,
                                   uint64_t iteration, double p, const int64_t* skip, int64_t nskip,
                                   float divisor, int32_t* idx, void* vals,
                                   int64_t cap, int64_t* count, void* work, hipStream_t stream);

/* ---- DeMo DCT codec ------------------------------------------------------ */

/*
 * One parameter tensor as the DeMo codec sees it: a 2-D [rows, cols] view of
 * the arena at `offset` (1-D [L] -> [1, L] with n1 = 1; 4-D [b,c,h,w] ->
 * [b*c*h, w] with n1 = h, n2 = w), cut into gy x gx chunks of n1 x n2
 * (demo_impl/demo.py:255-276).  Each chunk sends k entries
 * (k = clamp(topk, 1, n1*n2), demo.py:307-323) stored at payload entry
 * payload_off + chunk*k.  basis1/basis2 index the 64x64 basis tables
 * (zero padded; n = 1 is the identity).  chunk_start is the prefix sum of
 * gy*gx over the descriptor table.
 */
typedef struct ga_demo_tensor {
    int64_t offset;
    int64_t payload_off;
    int32_t rows, cols;
    int32_t n1, n2;
    int32_t gy, gx;
    int32_t k;
    int32_t basis1, basis2;
    int32_t chunk_start;
} ga_demo_tensor;

/* sizeof(ga_demo_tensor) as compiled into the library (ABI check for bindings). */
GA_API int ga_demo_tensor_bytes(void);

/*
 * Alignment, for the four DeMo entry points below (ga_demo_encode,
 * ga_demo_encode_sym, ga_demo_decode, ga_demo_decode_sym): param, grad and delta
 * may have any element alignment and any ld; the results are bit-identical
 * either way and nothing outside the rows is written.  The kernels use 4-element
 * vector accesses only when every arena base passed is 16 B (fp32) / 8 B (bf16)
 * aligned and, for K > 1, ld % 4 == 0 (per tensor also offset % 4 == 0 and
 * cols % 4 == 0, which an arena layout aligned to 64 elements gives); otherwise
 * they load and store element by element, which is slower.  The payload needs
 * only its natural 4 B alignment; payload_stride may be any value >= 2*M.
 *
 * Payload indices on decode: an entry whose index is outside the chunk's
 * coefficient range [0, n1*n2) -- negative or too large -- is ignored: it adds
 * neither its value nor a hit to any coefficient's mean.  (The encoders emit
 * only valid indices; a receiver does not have to validate gathered payloads.)
 */

/*
 * Encode + compress + residual for every chunk of every tensor, for each of
 * K replicas (replica r: param/grad/delta at + r*ld, payload at + r*payload_stride):
 *   p     *= wd_factor                      if wd_factor != 1 (demo.py:159-160; the
 *                                           caller passes 1 - lr*weight_decay computed
 *                                           in double, as the reference's Python scalar)
 *   delta  = decay*delta + lr*grad          (demo.py:163-167)
 *   Y      = F1^T . delta_chunk . F2        (DCT-II, demo.py:255-276; fp32 MFMA)
 *   top-k of |Y| per chunk                   (demo.py:315-328; ties: lowest index)
 *   delta -= B1^T . S . B2                  (S = the k kept coefficients, demo.py:174-180)
 * Payload per replica: idx int32[M] then val f32[M] (M = total entries), entries
 * of one chunk in ascending coefficient index.  F/B tables: [nbasis][64][64] fp32.
 */
GA_API int ga_demo_encode(int dtype, const ga_demo_tensor* tensors, int32_t ntensors,
                          int32_t nchunks, const float* F, const float* B,
                          void* param, const void* grad, void* delta, int64_t K,
                          int64_t ld, float lr, float decay, float wd_factor,
                          int32_t* payload, int64_t payload_stride, int64_t M,
                          hipStream_t stream);

/*
 * Up to 64 consecutive 1x64 chunks of one tensor (rows of a vector's chunk
 * view): element offset of the first chunk, payload entry offset of its
 * entries, number of chunks, entries per chunk.
 */
typedef struct ga_demo_rowgroup {
    int64_t offset;
    int64_t payload_off;
    int32_t rows;
    int32_t k;
} ga_demo_rowgroup;

/*
 * ga_demo_encode (demo.py:142-209 encode + compress + residual) for plans whose
 * chunks are all 64x64 or 1x64 with k <= 64 -- compression_chunk = 64 on
 * GPT-2-shaped models: same arithmetic, payload layout and tie rule.  The
 * 64x64 chunks are described by `tensors` (only 64x64 tensors, chunk_start
 * counting those chunks, payload_off as in the full plan), the 1x64 chunks by
 * `groups`; F64 is the 64-point basis F[i][k] (64x64 fp32).  One wavefront per
 * chunk (or row group), operands register-resident, the DCT products folded by
 * the symmetry F[63-i][k] = (-1)^k F[i][k].
 */
GA_API int ga_demo_encode_sym(int dtype, const ga_demo_tensor* tensors, int32_t ntensors,
                              int32_t nchunks, const ga_demo_rowgroup* groups, int32_t ngroups,
                              const float* F64, void* param, const void* grad, void* delta,
                              int64_t K, int64_t ld, float lr, float decay, float wd_factor,
                              int32_t* payload, int64_t payload_stride, int64_t M,
                              hipStream_t stream);

/*
 * Decode the gathered payloads of S sources (source s at payload + s*payload_stride,
 * in node order), scatter-mean them per chunk (mean over the entries that hit a
 * coefficient, demo.py:331-352), inverse DCT (B1^T . X . B2), sign, and apply the
 * SGD step to each of K local replicas:  grad = sign(g);  p -= lr*grad
 * (demo.py:192-209).  grad may be null (then only p is written).
 */
GA_API int ga_demo_decode(int dtype, const ga_demo_tensor* tensors, int32_t ntensors,
                          int32_t nchunks, const float* B, const int32_t* payload,
                          int64_t payload_stride, int64_t M, int64_t S, void* param,
                          void* grad, int64_t K, int64_t ld, float lr,
                          hipStream_t stream);

/*
 * ga_demo_decode for the plans ga_demo_encode_sym takes (64x64 chunks in
 * `tensors`, 1x64 chunks in `groups`, F64 the 64-point basis) and S <= 15
 * sources: same arithmetic and replica update as ga_demo_decode
 * (demo.py:192-209, 331-352), one wavefront per chunk or row group.  S == 1 is
 * a sparse synthesis of the k entries; S >= 2 scatter-adds the sources in node
 * order into an LDS tile with 4-bit hit counts, takes the mean over hitters and
 * runs the inverse transform as two folded 64-deep MFMA products.
 */
GA_API int ga_demo_decode_sym(int dtype, const ga_demo_tensor* tensors, int32_t ntensors,
                              int32_t nchunks, const ga_demo_rowgroup* groups, int32_t ngroups,
                              const float* F64, const int32_t* payload, int64_t payload_stride,
                              int64_t M, int64_t S, void* param, void* grad, int64_t K, int64_t ld,
                              float lr, hipStream_t stream);

/* ---- inner optimizer on the arena --------------------------------------- */

/* Number of fp32 partials ga_grad_clip_coef needs in its `partials` buffer. */
GA_API int ga_sumsq_partials_count(void);

/*
 * Gradient-norm clipping coefficient per replica k < K of a gradient replica set
 * (replica k: n elements at grad + k*ld):
 *   out[2k+1] = ||grad_k||_2 (fp32 partial sums in a fixed order), and
 *   out[2k]   = clamp(max_norm / (out[2k+1] + 1e-6), max = 1) as torch clamps:
 *               a NaN norm gives a NaN coefficient (never 1), an infinite norm 0.
 * `partials` holds K * ga_sumsq_partials_count() floats.  Device side only
 * (nothing synchronises); ga_adam_step applies out[2k] to replica k.
 * Replaces: torch.nn.utils.clip_grad_norm_(model.parameters(), max_norm) at
 * exogym/strategy/strategy.py:135-138, communicate_optimize_strategy.py:69-71,
 * diloco.py:52-56 (the per-tensor norms + stack + norm + per-tensor mul_).
 */
GA_API int ga_grad_clip_coef(int dtype, const void* grad, int64_t K, int64_t ld, int64_t n, float max_norm,
                             float* partials, float* out, hipStream_t stream);

/*
 * One fused Adam/AdamW step over K replicas of an fp32 arena (param, grad,
 * exp_avg, exp_avg_sq: [K, ld] sets, n elements per replica, 16-byte aligned),
 * every replica with the same hyper-parameters, in torch's op order
 * (torch/optim/adam.py, _multi_tensor_adam):
 *   g = grad * clip_coef[2k]  (and written back) if clip_coef != null and !(clip_coef[2k] >= 1):
 *                             a NaN coefficient scales too, so the replica's gradient, moments
 *                             and parameters become NaN as after clip_grad_norm_ + step()
 *   p *= wd_factor            (AdamW: 1 - lr*weight_decay, computed by the caller in double)
 *   g += l2_wd * p            (Adam with weight_decay)
 *   m = lerp(m, g, lerp_w)    (lerp_w = 1 - beta1)
 *   v = beta2*v + one_m_beta2*g*g
 *   p += step_size * m / (sqrt(v)/bc2_sqrt + eps)   (step_size = -lr/(1-beta1^t), bc2_sqrt = sqrt(1-beta2^t))
 * Replaces: `self.optim.step()` with the default inner optimizer
 * torch.optim.AdamW (exogym/strategy/strategy.py:140, diloco.py:59,
 * communicate_optimize_strategy.py:74; OptimSpec default optim.py:11).
 */
GA_API int ga_adam_step(int dtype, void* param, void* grad, float* exp_avg, float* exp_avg_sq, int64_t K,
                        int64_t ld, int64_t n, float lerp_w, float beta2, float one_m_beta2, float eps,
                        float wd_factor, float l2_wd, float step_size, float bc2_sqrt, const float* clip_coef,
                        hipStream_t stream);

/*
 * One fused SGD step (momentum, dampening, Nesterov, L2 weight decay) over K
 * replicas of an fp32 arena (param, grad, momentum_buf: [K, ld] sets, n elements
 * per replica, 16-byte aligned), every replica with the same hyper-parameters, in
 * torch's op order (torch/optim/sgd.py, _single_tensor_sgd / _multi_tensor_sgd):
 *   g = grad * clip_coef[2k]  (and written back) if clip_coef != null and !(clip_coef[2k] >= 1):
 *                             a NaN coefficient scales too (ga_adam_step's rule)
 *   g += weight_decay * p     (weight_decay != 0; not written back)
 *   momentum != 0:
 *     buf = g                                    if first (torch clones the first gradient: no dampening)
 *         | momentum*buf + one_m_dampening*g     otherwise
 *     g   = g + momentum*buf (nesterov) | buf
 *   p += neg_lr * g
 * neg_lr = -lr and one_m_dampening = 1 - dampening are computed by the caller in
 * double.  With momentum == 0 momentum_buf may be null and is neither read nor
 * written; with `first` set it is written and not read.  Bytes per element: 12
 * without momentum, 20 with, 16 on a first step, +4 when the clipped gradient is
 * written back.
 * Replaces: `self.optim.step()` with OptimSpec(torch.optim.SGD, ...), the "sgd" of
 * OptimSpec.from_string (exogym/strategy/optim.py:24; strategy.py:135-140,
 * diloco.py:52-59, communicate_optimize_strategy.py:69-74).
 */
GA_API int ga_sgd_step(int dtype, void* param, void* grad, float* momentum_buf, int64_t K, int64_t ld, int64_t n,
                       float neg_lr, float momentum, float one_m_dampening, float weight_decay, int nesterov,
                       int first, const float* clip_coef, hipStream_t stream);

/* ---- node drift: model correlation and consensus distance ---------------- */

/* Bytes of the `work` buffer ga_replica_gram needs for K replicas of n elements
 * (one fp32 partial of K*K + 2K values per workgroup); -1 for K outside 1..32 or n < 0. */
GA_API int64_t ga_replica_gram_workspace_bytes(int64_t K, int64_t n);

/* L: the most fused multiply-adds any fp32 accumulator of ga_replica_gram takes
 * before it is written out as a partial (<= 4096).  The fp32 error of a Gram entry
 * is first-order bounded by (L + 16) * 2^-24 * sum_e |x_i[e] x_j[e]|. */
GA_API int ga_replica_gram_chain(void);

/*
 * One read of a replica set src [K, ld] (K <= 32, n elements per row, f32 or bf16
 * widened to f32) gives, in fp64 on the device:
 *   gram[i*K + j] = sum_e x_i[e] * x_j[e]          (the full symmetric K x K matrix)
 *   rowsum[k]     = sum_e x_k[e]
 *   dist2[k]      = sum_e (x_k[e] - m[e])^2, m[e] = (fp32 sum of x_k[e] in ascending k) / K
 *                   with a true division (ga_replica_mean's rule); skipped if dist2 is null.
 * From gram and rowsum the host derives every pair's Pearson correlation; dist2 is
 * the squared distance of each node to the node mean (the consensus distance),
 * computed from centred values because gram_kk - 2 x_k.m + m.m cancels when the
 * nodes are close.  The Gram products run on the f32 MFMA (K <= 16: 16x16x4,
 * else 32x32x2, rows >= K fed zeros), fp32 partials per workgroup go to `work`
 * (ga_replica_gram_workspace_bytes) and a second kernel sums them in a fixed order
 * in fp64: no atomics, the same input gives the same bits.  Elements at index >= n
 * of a row (tail and ld - n padding) are never read.  16-byte vector loads (8-byte
 * for bf16) when src is so aligned and ld % 4 == 0, element loads otherwise, same
 * results.  n == 0 zeroes the (non-null) outputs.  K > 32: GA_EUNSUP.
 *
 * Replaces: exogym/train_node.py:498-573 (_correlation_calculation: every node's
 * state dict saved to disk, loaded on rank 0, np.corrcoef per pair; disabled in the
 * reference by a leading `return`), called from train_node.py:614-616.
 */
GA_API int ga_replica_gram(int dtype, const void* src, int64_t K, int64_t ld, int64_t n, double* gram,
                           double* rowsum, double* dist2, void* work, hipStream_t stream);

/* Bytes of the `work` buffer ga_replica_gram_centered needs (one fp32 partial of
 * K*K + 2K + 2 values per workgroup of 16384 columns); -1 for K outside 1..32 or n < 0. */
GA_API int64_t ga_replica_gram_centered_workspace_bytes(int64_t K, int64_t n);

/*
 * ga_replica_gram's one read of src [K, ld] (K <= 32, n elements per row, f32 or
 * bf16 widened to f32), taken over the centred values.  With
 *   m[e]   = (fp32 sum of x_k[e] in ascending k) / K   (true division, dist2's rule)
 *   d_k[e] = x_k[e] - m[e]                              (fp32)
 * it gives, in fp64 on the device:
 *   cgram[i*K + j] = sum_e d_i[e] * d_j[e]   (the full symmetric K x K matrix, f32 MFMA)
 *   mdot[k]        = sum_e m[e] * d_k[e]
 *   dsum[k]        = sum_e d_k[e]
 *   mstat[0]       = sum_e m[e]^2,  mstat[1] = sum_e m[e]
 * so x_i . x_j = mstat[0] + mdot[i] + mdot[j] + cgram[i*K + j] and sum x_k =
 * mstat[1] + dsum[k], but the large common part m is kept apart from the small
 * differences d: cgram_ii + cgram_jj - 2 cgram_ij is |x_i - x_j|^2 and the host's
 * 1 - corr_ij (gym_amd/metrics.py) stay accurate when the nodes are 1e-3 and less
 * apart, where gram_ii + gram_jj - 2 gram_ij and gram_ij - rowsum_i rowsum_j / n
 * cancel.  cgram[k*K + k] is ga_replica_gram's dist2[k].  The node mean of a column
 * is complete before any row of its tile is used; everything else is
 * ga_replica_gram's: MFMA shapes, fp32 partials in `work`
 * (ga_replica_gram_centered_workspace_bytes), the fixed-order fp64 final sum, no
 * atomics and the same bits for the same input, ga_replica_gram_chain() as the chain
 * bound L of every fp32 accumulator, elements at index >= n never read, 16-byte
 * (bf16: 8-byte) vector loads when src is so aligned and ld % 4 == 0 and element
 * loads otherwise with the same results.  n == 0 zeroes the (non-null) outputs;
 * otherwise all four are required.  K > 32: GA_EUNSUP.
 *
 * Replaces: exogym/train_node.py:498-573 (_correlation_calculation's np.corrcoef
 * per pair, which works in float64 and so resolves close nodes).
 */
GA_API int ga_replica_gram_centered(int dtype, const void* src, int64_t K, int64_t ld, int64_t n, double* cgram,
                                    double* mdot, double* dsum, double* mstat, void* work, hipStream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* GYM_AMD_H */
