/*
 * ava_hip.h -- C ABI of libava_hip.so: the MI355X (gfx950) implementation of the VAE
 * training hot path of pearsonlab/autoencoded-vocal-analysis (reference file
 * ava/models/vae.py).
 *
 * The reference has no FFI of its own (it is 100 % Python on top of torch); the entry
 * points below are what a binding for this path replaces, one per implicit library op
 * the reference dispatches, plus a fused whole-step driver.
 * Every function takes raw device pointers, sizes and a hipStream_t (passed as void*),
 * returns 0 on success or a negative AVA_E* code, allocates nothing and never
 * synchronises: all scratch memory comes from the caller-provided workspace.
 *
 * Layouts: activations are NHWC fp32 (`[B,H,W,C]`) between the convolutions, row-major
 * `[B,features]` on the fully connected side with the reference's NCHW flatten order
 * (c*256 + h*16 + w, vae.py:224,262) at the two boundaries.  Parameters live in ONE
 * flat fp32 arena in named_parameters() order (offsets: ava_param_offset), shadowed by
 * three arenas of the same shape for the gradient, Adam exp_avg and exp_avg_sq.
 */
#ifndef AVA_HIP_H
#define AVA_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define AVA_OK 0
#define AVA_EINVAL (-1)   /* bad argument (shape, null pointer, unsupported channel count) */
#define AVA_ELAUNCH (-2)  /* hipGetLastError() reported a launch failure                    */
#define AVA_EWORKSPACE (-3) /* workspace too small                                          */

typedef void* ava_stream_t;            /* hipStream_t */
typedef struct ava_model ava_model;    /* opaque: pointer table + workspace carving, host memory only */

/* ---- library / layout queries ------------------------------------------------------------- */
int ava_version(void);
/* number of floats of the flat parameter arena for this z_dim (tensors padded to 64 floats) */
int64_t ava_arena_floats(int z_dim);
/* offset (in floats) of parameter `index` (0..79, reference named_parameters() order,
 * vae.py:125-168) inside the arena; numel returned through *numel (may be NULL) */
int64_t ava_param_offset(int z_dim, int index, int64_t* numel);
/* bytes of scratch the model needs for batches up to max_batch */
size_t ava_workspace_bytes(int z_dim, int max_batch);

/* ---- model object: replaces VAE.__init__/_build_network bookkeeping (vae.py:80-168) -------- */
/* bn_running: [2][14][32] floats = running_mean then running_var of bn1..bn14, 32 slots per layer
 * (channel counts 1,8,8,16,16,24,24,32,24,24,16,16,8,8); bn_batches: 14 int64 counters. */
int ava_model_create(ava_model** out, int z_dim, int max_batch, float model_precision,
                     float* params, float* grads, float* exp_avg, float* exp_avg_sq,
                     float* bn_running, int64_t* bn_batches, void* workspace, size_t workspace_bytes);
void ava_model_destroy(ava_model* m);
/* The same for spectrograms of H x W instead of the reference's module constant X_SHAPE = (128, 128) (vae.py:33-36;
 * BASELINE config 5 is 256 x 256): every layer keeps its channels, strides and 3x3 kernels, the spatial sizes scale, and
 * fc1.in = fc8.out = 32 * (H/8) * (W/8) replaces the literal 8192 of vae.py:142,153,224,262.  W must be 128 or 256 and H
 * a multiple of 128 (128..1024); other sizes return -1 / 0 / AVA_EINVAL.  The functions without the _hw suffix are
 * these with H = W = 128. */
int64_t ava_arena_floats_hw(int z_dim, int H, int W);
int64_t ava_param_offset_hw(int z_dim, int H, int W, int index, int64_t* numel);
size_t ava_workspace_bytes_hw(int z_dim, int H, int W, int max_batch);
int ava_model_create_hw(ava_model** out, int z_dim, int H, int W, int max_batch, float model_precision,
                        float* params, float* grads, float* exp_avg, float* exp_avg_sq,
                        float* bn_running, int64_t* bn_batches, void* workspace, size_t workspace_bytes);
/* ... and with the storage type of the activations between the convolutions (BASELINE configs[4]: "bf16 conv + fp32
 * ELBO"): act_dtype 0 = float32 (the reference), 1 = bfloat16 -- the thirteen tensors that connect the 14 conv layers
 * (and are kept for the backward pass) are stored as bf16, rounded to nearest even by the producing kernel; every
 * product still accumulates in fp32 on the matrix cores / packed FMAs, and BatchNorm statistics (taken of the
 * rounded values), gradients, the fully connected layers, the ELBO and Adam (fp32 master weights) stay fp32.  Same
 * workspace size as ava_workspace_bytes_hw. */
int ava_model_create_ex(ava_model** out, int z_dim, int H, int W, int act_dtype, int max_batch, float model_precision,
                        float* params, float* grads, float* exp_avg, float* exp_avg_sq,
                        float* bn_running, int64_t* bn_batches, void* workspace, size_t workspace_bytes);

/* ---- whole-path entry points ------------------------------------------------------------------ */
/* VAE.forward (vae.py:273-327): encode -> rsample -> decode -> -ELBO.
 *   x [B,128,128]; eps_w [B], eps_d [B,z]: the two normal draws of rsample in reference order.
 *   bn_train: 1 = batch statistics + running-stat update (module.train()), 0 = running stats.
 *   loss_out (device, 4 floats): {-ELBO, sum z^2, SSE, sum entropy}.
 *   loss_accum (device double, may be NULL): -ELBO is also added to it (the epoch loops' running sum,
 *     vae.py:351,382, kept on the device so that no step needs a host sync).
 *   status_out (device int[2], may be NULL): word 0 is OR-ed with 1 when some d is not > 0 (reference raises
 *     ValueError); sticky -- the caller clears it after reading.  Word 1 is incremented by every ava_adam_step that
 *     skipped its update because word 0 was set (so the caller can take those steps back out of its step count).
 * x, eps_w, eps_d must stay valid until ava_backward has run.
 * Leaves every intermediate needed by ava_backward in the workspace, together with the BatchNorm mode: the backward of
 * a bn_train = 0 forward differentiates the running-statistics form (dx = gamma*invstd*g), as autograd does for
 * model.eval(); loss = model(x); loss.backward().  ava_encode / ava_decode overwrite those intermediates: an
 * ava_backward after them returns AVA_EINVAL until the next ava_forward. */
int ava_forward(ava_model* m, const float* x, int B, const float* eps_w, const float* eps_d,
                int bn_train, float* loss_out, double* loss_accum, int* status_out, ava_stream_t s);
/* The same with the noise of rsample() (vae.py:313) drawn by the device inside the forward's first launch instead of
 * being passed in: eps (device, B*(z_dim+1) floats) receives eps_W [B] then eps_D [B,z_dim], elements offset ..
 * offset + B*(z_dim+1) - 1 of the counter stream of ava_fill_normal(seed) -- bit-identical to ava_fill_normal(eps, ...)
 * followed by ava_forward(m, x, B, eps, eps + B, ...), one launch less.  eps must stay valid until ava_backward. */
int ava_forward_noise(ava_model* m, const float* x, int B, float* eps, uint64_t seed, uint64_t offset,
                      int bn_train, float* loss_out, double* loss_accum, int* status_out, ava_stream_t s);
/* loss.backward() (vae.py:352) for the forward that just ran: fills the gradient arena
 * (overwrites: the reference zero_grad()s before every step, vae.py:348). */
int ava_backward(ava_model* m, const float* x, int B, ava_stream_t s);
/* autograd hands loss.backward() a grad_output; when the caller backpropagates c*loss (or a sum the loss is part of)
 * it is not 1.  loss_scale: device pointer to that scalar, read by the NEXT ava_backward / ava_backward_part sequence
 * (the seed gradient and the prior/entropy terms are multiplied by it: the gradient is linear in it), then forgotten.
 * NULL (the default after every ava_forward) means 1.  Replaces a 70 MB pass over the gradient arena. */
int ava_set_backward_scale(ava_model* m, const float* loss_scale);
/* The same backward in ava_backward_num_parts() (= 4) consecutive parts, so that a data-parallel caller can
 * all-reduce each part's gradients while the next part runs.  Part p completes gradient bucket p, a contiguous
 * range of the arena returned by ava_grad_bucket (floats): bucket 0 = fc8, convt1..7, bn8..14 (tail of the arena),
 * bucket 1 = fc1.weight alone (the largest tensor: it goes out as soon as its product is enqueued), bucket 2 = fc1.bias,
 * fc2..fc7, bucket 3 = conv1..7, bn1..7 (head).  The buckets tile the arena. */
int ava_backward_num_parts(void);
int ava_backward_part(ava_model* m, const float* x, int B, int part, ava_stream_t s);
int ava_grad_bucket(ava_model* m, int bucket, int64_t* offset, int64_t* count);
/* Data parallelism (the reference is single-device: vae.py:112-115).  Every convolution / large-GEMM launch is ONE
 * resident wave of persistent workgroups over a static tile partition; a collective's own persistent workgroups (RCCL)
 * need wave slots beside them.  ava_set_cu_reserve(r) sizes all those grids for (256 - r) CUs from now on (process-wide,
 * 0 <= r <= 128; default 0).  Results are bit-reproducible for a given r.  ava_occupy_cus(w, lds, usec, stream) launches w
 * 256-thread workgroups with `lds` bytes of LDS each (which bounds how many share a CU) that only hold their slots for
 * usec microseconds (<= 20 ms): a stand-in for such a collective in tests. */
int ava_set_cu_reserve(int cus);
int ava_get_cu_reserve(void);
/* The same per model: the persistent grids of THIS model's entry points (forward, backward parts, encode, decode) are sized
 * for (256 - cus) CUs from the next call on; -1 (the default) follows the process-wide setting.  Adam is not affected: its
 * kernel is a grid-stride launch of small blocks with no static tile partition, which fills whatever wave slots a collective
 * leaves free and needs no co-residency.  Each entry point reads the
 * value once, at its start, so launches that hand partial rows to each other inside one call always agree on the grid. */
int ava_model_set_cu_reserve(ava_model* m, int cus);
int ava_model_get_cu_reserve(const ava_model* m);
int ava_occupy_cus(int workgroups, int lds_bytes, float usec, ava_stream_t s);
/* torch.optim.Adam.step (torch/optim/adam.py:414-547), one fused pass over the four arenas.
 * `step` is the 1-based count after increment.  When the last ava_forward raised its status word (some d not > 0: the
 * reference raises ValueError inside forward and never reaches optimizer.step(), vae.py:312,353) the kernel leaves
 * parameters and moments untouched. */
int ava_adam_step(ava_model* m, double lr, double beta1, double beta2, double eps, int step, ava_stream_t s);
/* The same update restricted to the floats [offset, offset + count) of the four arenas (offset, count multiples of 4):
 * a data-parallel caller that reduce-scatters the gradient buckets lets every rank update its 1/N slice of each bucket
 * and all-gathers the parameters (same bytes on the wire as an all-reduce, Adam's HBM traffic divided by N). */
int ava_adam_step_range(ava_model* m, int64_t offset, int64_t count, double lr, double beta1, double beta2, double eps,
                        int step, ava_stream_t s);
/* VAE.encode (vae.py:216-233): mu,u,d [B,z] (d = exp(.)); bn_train as above. */
int ava_encode(ava_model* m, const float* x, int B, int bn_train, float* mu, float* u, float* d, ava_stream_t s);
/* VAE.decode (vae.py:258-270): z [B,z] -> x_rec [B,16384]. */
int ava_decode(ava_model* m, const float* z, int B, int bn_train, float* x_rec, ava_stream_t s);
/* pointers into the workspace after ava_forward: z [B,z] and x_rec [B,16384] */
const float* ava_last_z(ava_model* m);
const float* ava_last_xrec(ava_model* m);
/* name -> workspace buffer of an intermediate (tests): "y1".."y7","d1".."d6","f8","mu","u","logd",... */
const float* ava_debug_buffer(ava_model* m, const char* name, int64_t* floats);

/* Optional timing of the driver's launches with HIP events recorded on the launch stream
 * (bench.py's roofline leg).  Categories, in order: conv forward, conv backward-data, conv weight-grad
 * (+ its reduction), BatchNorm statistics/finalise, GEMM, layout hand-offs, latent+ELBO, Adam, weight pack.
 * ava_profile_read adds elapsed milliseconds (and launch-group counts) per category and clears the list.
 * on = 1: an event after every launch group (~100 per step; the records stretch the step by 10-15 %).
 * on = 2: coarse pass, after at least one step was read in mode 1: events only where the kernel FAMILY changes
 * (conv + BatchNorm + pack vs everything else, ~20 per step); a run's time is added to the category of its last
 * launch group, so only the family sums are meaningful -- they are the un-stretched figures the roofline uses. */
#define AVA_PROFILE_CATEGORIES 9
int ava_profile_enable(ava_model* m, int on);
int ava_profile_read(ava_model* m, float* ms, int* launches);

/* ---- per-op entry points (what the reference reaches through ATen) ---------------------------- */
/* counter-based standard normals (replaces torch's normal_() in rsample when no noise is injected) */
int ava_fill_normal(float* out, int64_t n, uint64_t seed, uint64_t offset, ava_stream_t s);

/* pack a Conv2d weight [Cout,Cin,3,3] / ConvTranspose2d weight [Cin,Cout,3,3] into the
 * gather form G[9][Cin_g][Cout_g] used by the kernels.
 *   kind: 0 conv fwd, 1 convT stride-1 fwd, 2 convT stride-2 fwd,
 *         3 conv stride-1 bwd-data, 4 conv stride-2 bwd-data, 5 convT stride-1 bwd-data, 6 convT stride-2 bwd-data */
int ava_pack_conv_weight(const float* w, float* g, int c_first, int c_second, int kind, ava_stream_t s);

/* 3x3 gather convolution, NHWC.  mode: 0 same-resolution (conv s1 / convT s1 / their bwd-data),
 * 1 down x2 (conv s2 fwd, convT s2 bwd-data), 2 up x2 (convT s2 fwd, conv s2 bwd-data).
 * Prologue applied to the input while it is staged into LDS (zero padding is applied AFTER it):
 *   pro 0: v*pa[c] + pb[c]                      (BatchNorm apply, vae.py:217-223)
 *   pro 1: (in2 > 0) ? pa[c]*v + pb[c]*in2 + pc[c] : 0   (ReLU mask + BatchNorm backward, in2 = saved activation)
 *   pro 2: v
 * Epilogue:
 *   epi 0: + bias, optional ReLU, store, per-channel {sum, sum^2} partials (next BatchNorm's statistics);
 *          out2 (optional, stride-1 layers with >= 8 channels on both sides): a second copy in NCHW order
 *          [B][Cout][Ho][Wo], the flatten order nn.Linear reads after conv7 (vae.py:224)
 *   epi 1: store, per-channel {sum g, sum g*xhat} partials with xhat = (epi_x - mean)*invstd (BatchNorm backward sums)
 *   epi 2: + bias, store x_rec, r = x_rec - epi_x, store prec*r to out2, partial {sum r^2}  (vae.py:319-320)
 * partials: [ava_conv_grid(...)][2*Cout] floats. */
int ava_conv_grid(int B, int Ho, int Wo, int mode);
int ava_conv3x3(const float* in, const float* in2, const float* pa, const float* pb, const float* pc,
                const float* G, const float* bias, float* out, float* out2,
                const float* epi_x, const float* epi_mean, const float* epi_invstd, float* partials,
                int B, int Hi, int Wi, int Cin, int Cout, int mode, int pro, int epi, int relu, float prec,
                ava_stream_t s);
/* weight/bias gradient of the same gather convolution: dG[9][Cin][Cout] and db[Cout] partials per
 * workgroup ([grid][9*Cin*Cout + Cout]); x side uses prologue 0 (BatchNorm apply), dy side pro 1 or 2. */
int ava_conv3x3_wgrad(const float* x, const float* xa, const float* xb,
                      const float* dy, const float* dy2, const float* da, const float* db_, const float* dc,
                      float* partials, int B, int Hi, int Wi, int Cin, int Cout, int mode, int dy_pro,
                      ava_stream_t s);
int ava_conv_wgrad_grid(int B, int Ho, int Wo, int mode);
/* rows of `partials` that ava_conv3x3_wgrad actually writes for this shape (<= ava_conv_wgrad_grid, which sizes the
 * buffer): the matrix-core kernels launch one resident wave of workgroups.  Reduce exactly this many rows, or zero
 * the buffer first. */
int ava_conv_wgrad_rows(int B, int Hi, int Wi, int Cin, int Cout, int mode, int dy_pro);
/* Fused backward of one layer (autograd's conv backward behind loss.backward(), ava/models/vae.py:349): ONE pass over
 * x, dy (and dy2) produces what ava_conv3x3(pro 1|2, epi 1) in the backward-data pattern and ava_conv3x3_wgrad produce
 * separately -- dx = gradient w.r.t. the BatchNorm output [B,Hi,Wi,Cin], bn_partials [grid][2*Cin] = {sum dx,
 * sum dx*xhat} with xhat = (x - mean)*invstd, wg_partials [grid][9*Cin*Cout + Cout].  Gb = backward-data weights
 * (pack kinds 3..6).  grid = ava_conv_fused_grid(...); 0 means the shape has no fused instantiation and
 * ava_conv3x3_bwd_fused returns AVA_EINVAL for it.  Every layer of the model has one at every size the model accepts
 * (the model's backward runs nothing else).  The 1 -> 8 layer (first layer: nothing upstream) never forms dx: pass dx = NULL, the sums are exact. */
int ava_conv_fused_grid(int B, int Hi, int Wi, int Cin, int Cout, int mode);
int ava_conv3x3_bwd_fused(const float* x, const float* xa, const float* xb,
                          const float* dy, const float* dy2, const float* da, const float* db_, const float* dc,
                          const float* Gb, float* dx, const float* mean, const float* invstd,
                          float* bn_partials, float* wg_partials,
                          int B, int Hi, int Wi, int Cin, int Cout, int mode, int dy_pro, ava_stream_t s);
/* reduce the per-workgroup partials and scatter into the reference weight layout
 * (kind as in ava_pack_conv_weight, 0..2 only) */
int ava_conv_wgrad_reduce(const float* partials, int nparts, float* dw, float* dbias,
                          int Cin, int Cout, int kind, ava_stream_t s);

/* BatchNorm2d statistics of a raw tensor [n, C] (channel innermost) -> partials [grid][2C] */
int ava_bn_stats(const float* x, int64_t n, int C, float* partials, int* nparts, ava_stream_t s);
/* partials -> mean, invstd, scale = gamma*invstd, shift = beta - mean*scale; train: running-stat update
 * (momentum 0.1, unbiased variance, eps 1e-5); eval: uses running stats. */
int ava_bn_finalize(const float* partials, int nparts, int64_t n, int C, const float* gamma, const float* beta,
                    float* running_mean, float* running_var, int64_t* num_batches, int train,
                    float* mean, float* invstd, float* scale, float* shift, ava_stream_t s);
/* backward: partials {sum g, sum g*xhat} -> dgamma, dbeta and the per-channel coefficients
 * dx = A*g + Bc*x + Cc */
int ava_bn_finalize_bwd(const float* partials, int nparts, int64_t n, int C, const float* gamma,
                        const float* mean, const float* invstd, float* dgamma, float* dbeta,
                        float* A, float* Bc, float* Cc, ava_stream_t s);

/* ---- test entry points of the training step's layout hand-offs and its BatchNorm accumulator ---------------------------
 * The launchers the model driver calls between the convolutional and the fully connected part, on caller-owned device
 * buffers (the ava_gemm_path precedent: nothing but tests calls these).  Tensors are [B][32][P] floats, P = pixels per
 * sample; "NCHW" is element b*32*P + c*P + p, "NHWC" element b*32*P + p*32 + c.  One workgroup moves tiles of 32 channels
 * x 64 pixels; tile w = b*(P/64) + q goes to workgroup w mod grid, grid = min((P/64)*B, 1024) for the statistics kernel
 * and min(.., 2048) for the others.  Every call returns AVA_EINVAL before any launch for a null pointer that is not
 * marked optional, B < 1, P < 64, P % 64 != 0 or act_bf16 outside {0, 1}.
 *
 * An accumulator slot is ava_acc_shards() shards of ava_acc_shard_ll() int64 words: [3 limbs][64 values] and a flag word
 * at 192.  Value idx of the slot is sum over shards of (limb0 + limb1 * 2^32 + limb2 * 2^64) * 2^-48, NaN when any flag
 * word is non-zero; a producer adds trunc(|p| * 2^48) of its fp32 partial p, split into three 32-bit limbs that carry the
 * sign of p, to shard (workgroup index mod shards), and sets the flag for a NaN, an Inf or |p| >= 2^47. */
int ava_acc_shards(void);
int ava_acc_shard_ll(void);
/* NCHW `in` -> NHWC `out` (stored as float, or as bfloat16 bits in the low half of the buffer when act_bf16) and the
 * per-channel {sum, sum of squares} of what was stored: to slot acc_out when it is not NULL (which = 0: sums at values
 * 0..31, squares at 32..63), else to partials [nparts][64].  slab1 != NULL: `in` is slab 0 of a two-slab product and the
 * element is 0 + in + slab1 (+ bias [32*P], optional), ReLU when relu = 1, also written to `full` (NCHW, optional).
 * slab1 == NULL requires bias = full = NULL and relu = 0.  nparts receives the grid. */
int ava_layout_nchw_to_nhwc_stats(const float* in, const float* slab1, const float* bias, int relu, float* full,
                                  float* out, float* partials, long long* acc_out, int B, int P, int act_bf16,
                                  int* nparts, ava_stream_t s);
/* NHWC `in` -> NCHW `out` */
int ava_layout_nhwc_to_nchw(const float* in, float* out, int B, int P, ava_stream_t s);
/* du (NHWC) = y_nhwc > 0 ? dy : 0 with dy the NCHW tensor dy_nchw, or 0 + dy_nchw + slab1 when slab1 (optional) is given */
int ava_layout_relu_mask_to_nhwc(const float* dy_nchw, const float* slab1, const float* y_nhwc, float* du, int B,
                                 int P, ava_stream_t s);
/* out (NCHW) = f > 0 ? fma(A[c], g, fma(Bc[c], f, Cc[c])) : 0 with g NHWC and f the stored value of f8 (NCHW; rounded to
 * bfloat16 when act_bf16).  acc == NULL: the coefficients are the arrays A, Bc, Cc [32].  acc != NULL: they are finalised
 * from slot acc ({sum g, sum g*xhat}) as ava_bn_finalize_bwd does from its partials, with Bc = Cc = 0 when eval = 1, zero
 * beyond C; workgroup 0 publishes dgamma [C], dbeta [C] and abc [3][32]; A, Bc, Cc are not read.  1 <= C <= 32, n >= 1. */
int ava_layout_bn_bwd_apply_to_nchw(const float* g, const float* f8, const float* A, const float* Bc, const float* Cc,
                                    float* out, int B, int P, int act_bf16, const long long* acc, const float* gamma,
                                    const float* mean, const float* invstd, float* dgamma, float* dbeta, float* abc,
                                    double n, int C, int eval, ava_stream_t s);
/* seed [n] (n >= 4, n % 4 == 0), wg [nwg] (optional; nwg >= 1 with it, nwg >= 0 without) and the 64 values of slot
 * (optional) times scale[0] (device), in place; the slot is rewritten as exact limbs in shard 0, a poisoned one as the flag
 * of shard 0.  scale[0] == 1 touches nothing. */
int ava_layout_scale_backward_roots(float* seed, int64_t n, float* wg, int64_t nwg, long long* slot,
                                    const float* scale, ava_stream_t s);

/* C[M,N] = relu_mask(act(A*B + bias)) on the fp32 matrix cores (nn.Linear and its two backward products).
 *   a_kmajor: 1 = A stored [M,K] (K contiguous), 0 = A stored [K,M] ; lda = stored leading dimension (0: dense)
 *   b_kmajor: 1 = B stored [N,K] (K contiguous), 0 = B stored [K,N] ; ldb likewise ; ldc: row stride of C (0: N)
 *   act: 0 none, 1 ReLU, 2 exp ; bias may be NULL ; split-K partial slabs go to `ws`
 *   mask (may be NULL, row stride ldc): C = mask > 0 ? value : 0  (ReLU backward of the layer that produced mask)
 *   colsum (may be NULL): receives sum over K of A (bias gradient when A = dY^T) */
size_t ava_gemm_workspace_bytes(int M, int N, int K);
int ava_gemm(const float* A, int lda, const float* B, int ldb, const float* bias, float* C, int ldc,
             const float* mask, float* colsum, int M, int N, int K, int a_kmajor, int b_kmajor, int act,
             void* ws, size_t ws_bytes, ava_stream_t s);
/* `ws` must be 16-byte aligned whenever the product is split (AVA_EWORKSPACE otherwise).
 *
 * Which kernel ava_gemm runs for these arguments: the dispatcher's own decision, taken on the host from shapes,
 * flags, pointer values and nullness alone (nothing is dereferenced or launched, no device is needed).
 * Returns 1 = three-limb bf16 kernel, 2 = skinny 16x16 kernel, 3 = LDS-tiled kernel, or AVA_EINVAL for arguments
 * ava_gemm refuses.  info (may be NULL) receives {tile (BN of the limb kernel, 16 for the skinny one, BM = BN of
 * the tiled one), K step of the instantiation, 16-byte operand loads (0/1; skinny: any k-major operand),
 * splits, K elements per split, threads per workgroup}. */
int ava_gemm_path(const float* A, int lda, const float* B, int ldb, const float* bias, const float* C, int ldc,
                  const float* mask, const float* colsum, int M, int N, int K, int a_kmajor, int b_kmajor, int act,
                  int* info);

/* latent block: d = exp(a), z = mu + u*eps_w + sqrt(d)*eps_d, per-sample sum z^2 and entropy
 * (torch/distributions/lowrank_multivariate_normal.py:17-38,214-252).  sums: [B][2]. */
int ava_latent_fwd(const float* mu, const float* u, const float* logd, const float* eps_w, const float* eps_d,
                   float* d, float* z, float* sums, int* status, int B, int zdim, ava_stream_t s);
/* closed-form backward: g = z + dz_dec */
int ava_latent_bwd(const float* z, const float* dz_dec, const float* u, const float* d, const float* eps_w,
                   const float* eps_d, float* dmu, float* du, float* dlogd, int B, int zdim, ava_stream_t s);
/* assemble -ELBO from the partial sums (vae.py:316-323); loss_out = {loss, sum z^2, SSE, sum H} */
int ava_elbo_finalize(const float* latent_sums, int B, const float* sse_partials, int nparts,
                      int zdim, float prec, float* loss_out, ava_stream_t s);
/* Adam over flat arenas */
/* hyper-parameters are doubles like the Python floats torch receives; each is rounded to fp32 exactly where
 * torch's kernels round it (1-beta1, beta2, 1-beta2, lr/bias_correction1, sqrt(bias_correction2), eps) */
int ava_adam_flat(float* p, const float* g, float* m, float* v, int64_t n, double lr, double beta1, double beta2,
                  double eps, int step, ava_stream_t s);

/* ---- input feeding ------------------------------------------------------------------- */
/* Loader bytes -> fp32 spectrograms on the device: replaces the per-item CPU conversion numpy_to_tensor
 * (ava/models/utils.py:444-446, applied by SyllableDataset.__getitem__, ava/models/vae_dataset.py:125-145) with a
 * device-side cast of the raw batch, same rounding as torch's .type(torch.FloatTensor).
 * src_dtype: 0 float32 (copy), 1 float64, 2 uint8, 3 float16, 4 bfloat16.  src and dst 16-byte aligned device
 * pointers, n elements. */
int ava_cast_to_f32(const void* src, int src_dtype, int64_t n, float* dst, ava_stream_t s);
/* HOST function (no GPU involved): collate a batch into a page-locked ring slot -- dst[i] = src[idx[i]] for n rows of
 * row_bytes each on `threads` host threads (idx == NULL: the contiguous rows first .. first+n-1).  Replaces the
 * per-item collation of the reference's DataLoader (ava/models/vae_dataset.py:89-96) for array-backed datasets. */
int ava_host_gather_rows(void* dst, const void* src, const int64_t* idx, int64_t first, int64_t n, size_t row_bytes,
                         int threads);
/* Row gather with the cast, on the device: dst[j, :] = float(src[idx[j], :]) for j < n, the
 * per-step path of a dataset that is resident in HBM (replaces SyllableDataset.__getitem__ + numpy_to_tensor + the
 * DataLoader's collation, ava/models/vae_dataset.py:125-145).  src: [n_rows][row_elems] of src_dtype (the codes of
 * ava_cast_to_f32, same rounding); idx: n int64 row numbers ON THE DEVICE, in any order, repeats allowed; dst:
 * [n][row_elems] float32.  16-byte loads and stores when a row is a whole number of 16-byte source vectors and of
 * float4s and src and dst are 16-byte aligned, one element per lane otherwise (any alignment the dtype allows).  A
 * row whose index is outside [0, n_rows) is neither read nor written.  Null pointers, n <= 0, n_rows <= 0,
 * row_elems <= 0 and an unknown dtype return AVA_EINVAL before any launch. */
int ava_gather_rows_f32(const void* src, int src_dtype, int64_t n_rows, int64_t row_elems, const int64_t* idx, int64_t n,
                        float* dst, ava_stream_t s);

/* ---- MMD^2 between sets of latent means (downstream consumer of get_latent) ------------ */
/* The Gaussian-kernel estimators of ava/plotting/mmd_plots.py (Gretton et al. 2012), bandwidth sigma: the unbiased
 * quadratic-time one of _estimate_mmd2 (:255-296) and the linear-time one of _estimate_mmd2_linear_time (:299-312),
 * for every pair of C conditions in one launch sequence -- the condition-by-condition loop of _calculate_mmd2
 * (:395-418, row f16).  One pair of index lists is the call with C = 2.
 * latent: [N][z] float64 row-major on the device (what VAE.get_latent returns, vae.py:538).  idx (device): the int64
 * index lists of the C conditions (already subsampled if the caller wants max_n), concatenated in condition order;
 * offsets (HOST) and offsets_dev (device): the same C + 1 int64 list starts, offsets[C] = len(idx).  2 <= C <= 4096,
 * every condition has 2 .. 2^31 - 1 rows (the reference divides by n (n - 1)), 1 <= z <= 128, sigma > 0 (AVA_EINVAL
 * otherwise).  k(x, y) = exp(-|x - y|^2 / (2 sigma^2)).
 * A table row is 4 int64 {first workgroup, first workspace slot, a, b}, followed by one sentinel row {total
 * workgroups, total slots, 0, 0}; with t_c = ceil(n_c / 64):
 *   blocks (ava_mmd2_matrix): the C (C + 1) / 2 blocks a <= b, row-major; block (a, b) has t_a t_b slots (its whole
 *     row-major tile grid) and t_a t_b workgroups, a symmetric block (a, a) t_a (t_a + 1) / 2 workgroups (the tiles on
 *     and above the diagonal);
 *   pairs (ava_mmd2_matrix_linear): the C (C - 1) / 2 pairs a < b, row-major; pair (a, b) has
 *     min(ceil(m / 256), 1024) workgroups and as many slots, m = min(n_a, n_b) / 2.
 * total_tiles / total_workgroups: column 0 of the sentinel row; it is checked against the host offsets and must be
 * below 2^31.  ws: ava_mmd2_matrix_workspace_bytes(offsets, C, linear) = (total slots + 8) doubles; returns 0 for
 * arguments the entry points reject.
 * ava_mmd2_matrix: within[a] (device, C doubles) = 2 / (n_a (n_a - 1)) sum_{i<j} k (term_1 / term_2 of :276-288),
 * cross (device, C x C doubles) [a][b] = [b][a] = 2 / (n_a n_b) sum k (term_3, :289-294), cross[a][a] = 0; the
 * estimate of a pair is within[a] + within[b] - cross[a][b], which the caller forms.
 * ava_mmd2_matrix_linear: out (device, C x C doubles) [a][b] = [b][a] = 1 / m sum_{i<m} h over the quadruples (x1, y1,
 * x2, y2) = rows (ia[2i], ib[2i], ia[2i+1], ib[2i+1]) of the two lists, h = k(x1,x2) + k(y1,y2) - k(x1,y2) - k(x2,y1):
 * the first 2 m indices of both lists; the diagonal is not written.  Neither allocates nor synchronises.
 * Every sum has one fixed order (no atomics), so a block's bits depend on its two lists, z and sigma alone, not on the
 * other conditions of the call.  First stage, one slot per workgroup of 256 threads = 4 waves: a tile's thread adds
 * its 4 x 4 pairs row by row (a pair's |x - y|^2 in the order of csrc/sqdist_tile.h), a pair's thread t of workgroup w
 * of W its quadruples w 256 + t, + 256 W, ...; then the wave sums r0 .. r3, then (r0 + r1) + (r2 + r3).  Second stage,
 * one workgroup per block or pair: thread t adds the slots t, t + 256, ... of the row-major grid (those below the
 * diagonal of a symmetric block left out), then the wave sums, then (r0 + r1) + (r2 + r3), then ONE multiply by
 * 2 / (n (n - 1)), 2 / (n_a n_b) or 1 / m. */
size_t ava_mmd2_matrix_workspace_bytes(const int64_t* offsets, int C, int linear);
int ava_mmd2_matrix(const double* latent, int z, const int64_t* idx, const int64_t* offsets, const int64_t* offsets_dev,
                    int C, const int64_t* blocks, int64_t total_tiles, double sigma, double* within, double* cross,
                    void* ws, size_t ws_bytes, ava_stream_t s);
int ava_mmd2_matrix_linear(const double* latent, int z, const int64_t* idx, const int64_t* offsets,
                           const int64_t* offsets_dev, int C, const int64_t* pairs, int64_t total_workgroups,
                           double sigma, double* out, void* ws, size_t ws_bytes, ava_stream_t s);
/* Permutation test for MMD^2 (row f18; Gretton et al. 2012, section 5; the model is DESIGN.md section 1 row f18).
 * A problem is a pair of index lists idx[o1 .. o1 + n1) and idx[o2 .. o2 + n2) (idx: device int64, n_idx entries); its
 * pool is their concatenation, positions j = 0 .. n1 + n2 - 1.  Split 0 is the caller's own (set 1 = positions
 * 0 .. n1 - 1); in split p >= 1 set 1 is the n1 positions with the smallest (key, j), key = the 64 hashed bits of
 * ava_amd.synthetic.u01 for element j of stream salt = ((seed + pair) mod 2^32) 2^32 + p.
 * table (HOST) and table_dev (device): n_problems + 1 rows of 8 int64 {o1, o2, n1, n2, pair, first position, first
 * row tile, 0}; "first position" is the sum of n1 + n2 and "first row tile" the sum of ceil((n1 + n2) / 64) over the
 * rows before; the last row is the sentinel {0, 0, 0, 0, 0, all positions, all row tiles, 0}.  A single test is a
 * table of one problem with pair = 0.
 * A call computes the splits p0 <= p < p1 of every problem:
 *   membership (device, (p1 - p0) x all positions bytes): [p - p0][first position + j] = 1 if j is in set 1
 *   terms (device, [n_problems][p1 - p0][3] doubles): term_1, term_2, term_3 of mmd_plots.py:277-295 for the split
 *   stats (device, [n_problems][p1 - p0] doubles): term_1 + term_2 - term_3
 *   stat0 (device, n_problems doubles), counts (device, n_problems int64): the call with p0 = 0 stores the statistic
 *     of split 0 and sets counts = #{p >= 1 in the call : stat_p >= stat_0}; a call with p0 > 0 reads stat0 and adds
 *     its count.  After the calls that cover 0 .. P, pvalue = (1 + counts) / (P + 1).
 * A split's values do not depend on how 0 .. P is cut into calls, nor on the other problems of the table.
 * ws: ava_mmd2_perm_workspace_bytes(table, n_problems, p1 - p0) = all row tiles x (p1 - p0 + 1) x 2 doubles + 256;
 * returns 0 for arguments the entry points reject.  ava_mmd2_perm_membership writes the bytes only (what the tests
 * compare); ava_mmd2_perm_tile() is the number of columns a workgroup of the statistic kernel owns.
 * AVA_EINVAL: n1 or n2 < 2, n1 + n2 > 2^24, more than 2^23 problems, a list that leaves idx, z outside 1 .. 128,
 * sigma not > 0, p0 < 0, p1 <= p0, p1 > 2^31 - 1, p1 - p0 > 2^20, n_problems (p1 - p0) > 2^31 - 1, a table whose sums
 * disagree; AVA_EWORKSPACE: ws too small.  Neither allocates nor synchronises. */
int ava_mmd2_perm_tile(void);
size_t ava_mmd2_perm_workspace_bytes(const int64_t* table, int n_problems, int n_splits);
int ava_mmd2_perm_membership(const int64_t* table, const int64_t* table_dev, int n_problems, int64_t p0, int64_t p1,
                             uint64_t seed, uint8_t* membership, ava_stream_t s);
int ava_mmd2_perm(const double* latent, int z, const int64_t* idx, int64_t n_idx, const int64_t* table,
                  const int64_t* table_dev, int n_problems, int64_t p0, int64_t p1, uint64_t seed, double sigma,
                  uint8_t* membership, double* terms, double* stats, double* stat0, int64_t* counts, void* ws,
                  size_t ws_bytes, ava_stream_t s);
/* squared distances of n index pairs, out[p] = |latent[a[p]] - latent[b[p]]|^2: the sampled pairs of
 * estimate_median_sigma (mmd_plots.py:450-474; the median itself is taken by the caller). */
int ava_pair_sqdist(const double* latent, int z, const int64_t* a, const int64_t* b, int n, double* out,
                    ava_stream_t s);

/* ---- shotgun spectrograms on the device -------------------------------------------
 * get_spec (ava/preprocessing/utils.py:18-110) for a batch of n windows as FixedWindowDataset.__getitem__ issues it
 * (ava/models/window_vae_dataset.py:213-224: get_spec(max(0, onset - shoulder), offset + shoulder, audio[file], p,
 * fs=fs, target_times=linspace(onset, offset, T))), with the audio of all files resident in ONE device buffer.
 *   audio / audio_dtype   concatenated samples of all files; 0 = int16, 1 = int32, 2 = float32, 3 = float64
 *                         (what scipy.io.wavfile.read returns, window_vae_dataset.py:167)
 *   file_off, file_len    [files] first sample / number of samples of each file in `audio` (device)
 *   file_idx, t1, t2      [n] file of each window, get_spec's t1 / t2 in seconds (device)
 *   target_times          [n][T] get_spec's target_times (device); target_freqs [F] (utils.py:80-88, device)
 *   max_samples           >= max over windows of round(t2 fs) - round(t1 fs): sizes the STFT scratch
 *   window, scale         scipy.signal.get_window('hann', nperseg) (device) and sqrt(1 / sum(window)^2): what
 *                         scipy.signal.stft(..., scaling='spectrum') applies (utils.py:74)
 *   spec_min, spec_max    p['spec_min_val'], p['spec_max_val'] (utils.py:100-103); fill_value utils.py:19
 *   out [n][F][T] fp32    the clipped spectrograms; out_max [n] or NULL: their maxima (min_spec_val test,
 *                         window_vae_dataset.py:229-231)
 *   normalize, q_lo,      p['within_syll_normalize'] (utils.py:104-108): subtract np.quantile(spec, p['normalize_quantile']),
 *   q_gamma               floor at 0, divide by max + 1e-12; the quantile is a[q_lo] + (a[q_lo+1] - a[q_lo]) * q_gamma over the
 *                         sorted F*T values (numpy's 'linear' method: q_lo and q_gamma as numpy derives them from q and F*T)
 * nperseg: 64..2048 (a power of two: radix-2 transform; any other length: direct fp64 transform of the needed bins, as
 * scipy.signal.stft takes any length, ava/preprocessing/utils.py:66-68), 0 <= noverlap < nperseg; T <= 512.
 * All arithmetic is fp64.  Windows the reference answers with zeros (utils.py:68-69) come out as zeros. */
size_t ava_spec_workspace_bytes(int n, int max_samples, int nperseg, int noverlap, int F, int T, int normalize);
int ava_get_spec_batch(const void* audio, int audio_dtype, const int64_t* file_off, const int64_t* file_len,
                       const int32_t* file_idx, const double* t1, const double* t2, const double* target_times,
                       int n, int max_samples, double fs, int nperseg, int noverlap, const double* window,
                       double scale, const double* target_freqs, int F, int T, double spec_min, double spec_max,
                       double fill_value, int remove_dc, int normalize, int q_lo, double q_gamma, float* out,
                       float* out_max, void* ws, size_t ws_bytes, ava_stream_t s);

/* ---- amplitude segmentation on the device -------------------------------------------
 * ava/segmenting/amplitude_segmentation.py:get_onsets_offsets for every file of a concatenated audio buffer at once.
 * The host keeps the greedy onset / offset chain and the duration filter (O(#maxima) integers); every per-frame step
 * runs here.
 *
 * ava_amp_workspace_bytes: scratch ava_amp_trace needs for `frames` frames in all (0 for frames <= 0).
 *
 * ava_amp_trace: the smoothed amplitude trace of every file.
 *   audio / audio_dtype   concatenated samples; 0 = int16, 1 = int32, 2 = float32, 3 = float64
 *   file_off, file_len    [files] first sample / number of samples of each file in `audio` (device)
 *   frame_off             [files + 1] first frame of each file in the concatenated trace (device); a file of
 *                         L >= nperseg samples has ceil(L / (nperseg - noverlap)) + 1 frames (scipy.signal.stft with
 *                         boundary='zeros', padded=True), a shorter one 0; frame_off[files] = frames
 *   nperseg, noverlap     a power of two in 64..2048, 0 <= noverlap < nperseg
 *   window, scale         get_window('hann', nperseg) (device), 1 / sum(window): 'spectrum' scaling; no detrend
 *   k0, k1                the kept bins [searchsorted(f, min_freq), searchsorted(f, max_freq)), 0 <= k0 < k1 <= nperseg/2+1
 *   spec_min, spec_max    v = clip((log(|X| + 1e-9) - spec_min) / (spec_max - spec_min), 0, 1)  (segmenting/utils.py:52-57)
 *   softmax, temperature  per frame sum v (softmax 0) or sum v e / (sum e + 1e-9), e = exp(v / temperature)
 *   gauss_w, radius       [2 radius + 1] gaussian_filter weights (device, host-normalised); radius 0 with w = {1}:
 *                         no smoothing.  Mode 'reflect' inside each file.
 *   trace_f64, trace      [frames] output, float64 (trace_f64 != 0) or float32: the dtype the reference holds
 *   spec                  [k1 - k0][frames] float64 band spectrogram (v) or NULL
 * All spectral arithmetic is fp64.
 *
 * ava_amp_decide: the decisions on a trace of `frames` values (float64 or float32, as trace_f64 says) split into
 * files by frame_off [files + 1] (device).  th1..th3 are compared against the trace values promoted to fp64: the caller
 * rounds them as numpy would compare them with the trace.  Writes *count (device) maxima: maxima[e] the global frame of
 * a local maximum (1 <= i <= T-2, a[i] > th3, a[i] == max(a[i-1:i+2])), left[e] / right[e] the nearest frame of its file
 * (>= 1 on the left, <= T-1 on the right) with a[j] < th1, or a[j] < th2 and a[j] == min(a[j-1:j+2]); -1 for none.
 * The order of the entries is not specified.  capacity >= frames.
 *
 * Both return AVA_EINVAL before any launch for null pointers, an unsupported nperseg, noverlap >= nperseg, an empty
 * band or a workspace that is too small. */
size_t ava_amp_workspace_bytes(int64_t frames);
int ava_amp_trace(const void* audio, int audio_dtype, const int64_t* file_off, const int64_t* file_len,
                  const int64_t* frame_off, int files, int64_t frames, int nperseg, int noverlap, const double* window,
                  double scale, int k0, int k1, double spec_min, double spec_max, int softmax, double temperature,
                  const double* gauss_w, int radius, int trace_f64, void* trace, double* spec, void* ws,
                  size_t ws_bytes, ava_stream_t s);
int ava_amp_decide(const void* trace, int trace_f64, const int64_t* frame_off, int files, int64_t frames, double th1,
                   double th2, double th3, uint64_t* count, int64_t* maxima, int64_t* left, int64_t* right,
                   int64_t capacity, ava_stream_t s);

/* ---- template segmentation on the device --------------------------------------------
 * The arithmetic core of ava/segmenting/template_segmentation.py:_segment_file for every file of a concatenated audio
 * buffer at once: the band spectrogram of _get_spec and the normalised cross-correlation with a template.  The host
 * keeps the threshold, the maxima and _clean_max_indices (O(lags) per file).
 *
 * ava_tpl_workspace_bytes: scratch ava_tpl_xcorr needs for `lags` lags in all (0 for lags <= 0).
 * ava_tpl_tile_lags: lags per correlation tile; the caller sizes tile_off with it.
 *
 * ava_tpl_spec: the band spectrogram and its per-frame sums: ava_amp_trace's band stage in sum mode, without smoothing.
 *   audio ... frame_off   as ava_amp_trace (0 = int16, 1 = int32, 2 = float32, 3 = float64; frame_off [files + 1])
 *   nperseg, noverlap     a power of two in 64..2048, 0 <= noverlap < nperseg
 *   window, scale         get_window('hann', nperseg) (device), 1 / sum(window): 'spectrum' scaling; no detrend
 *   k0, k1                the kept bins [searchsorted(f, min_freq), searchsorted(f, max_freq)), 0 <= k0 < k1 <= nperseg/2+1
 *   spec_min, spec_max    S = clip((log(|X| + 1e-9) - spec_min) / (spec_max - spec_min), 0, 1)  (template_segmentation.py:786-789)
 *   spec                  [k1 - k0][frames] float64 output, frequency-major
 *   frame_sum             [frames] float64 output: sum over the band of each frame, in a fixed order
 *
 * ava_tpl_xcorr: the trace [lags] float64 of every file.
 *   spec, frame_sum, F    what ava_tpl_spec wrote (F = k1 - k0 rows of `frames` frames)
 *   frame_off             [files + 1] as above (device)
 *   lag_off               [files + 1] first lag of each file in the trace (device): n_f - L lags for a file of n_f frames
 *                         that is segmented, 0 for one that is skipped; lag_off[files] = lags
 *   tile_off              [files + 1] first workgroup of each file (device): file f has ceil(lags_f / ava_tpl_tile_lags())
 *                         tiles; tile_off[files] = tiles
 *   tmpl, template_F, L   the template [template_F][L] float64 (device); template_F must equal F
 *   trace                 r_i = N_i / (Q_i + 1e-9), N_i = sum T[k,t] (S[k,i+t] - mu_i), Q_i = sum (S[k,i+t] - mu_i)^2,
 *                         mu_i = the mean of S over frames i..i+L-1 (template_segmentation.py:240-245).  Every lag's
 *                         sums run in one fixed order: the trace is bit-reproducible and does not depend on the other
 *                         files of the launch.
 * All arithmetic is fp64.  Both return AVA_EINVAL before any launch for null pointers, an unsupported nperseg,
 * noverlap >= nperseg, an empty band, L <= 0, template_F != F or a workspace that is too small. */
size_t ava_tpl_workspace_bytes(int64_t lags);
int ava_tpl_tile_lags(void);
int ava_tpl_spec(const void* audio, int audio_dtype, const int64_t* file_off, const int64_t* file_len,
                 const int64_t* frame_off, int files, int64_t frames, int nperseg, int noverlap, const double* window,
                 double scale, int k0, int k1, double spec_min, double spec_max, double* spec, double* frame_sum,
                 ava_stream_t s);
int ava_tpl_xcorr(const double* spec, const double* frame_sum, int F, int64_t frames, const int64_t* frame_off,
                  const int64_t* lag_off, const int64_t* tile_off, int files, int64_t lags, int64_t tiles,
                  const double* tmpl, int template_F, int L, double* trace, void* ws, size_t ws_bytes, ava_stream_t s);

/* ---- time-warped shotgun windows on the device -------------------------------------
 * WarpedWindowDataset (ava/models/window_vae_dataset.py:358-701) draws windows of song motifs under per-file piecewise
 * linear time warps; every window is get_spec(0.0, template_dur, audio[file], p, fs=fs, target_times=...).  The slice,
 * its mean and its log-spectrogram are the same for every window of a file: ava_warp_cache_build makes them once for
 * all files (the kernels of ava_get_spec_batch, run with one window per file), ava_warp_windows interpolates a batch out
 * of that cache with the interpolation and normalisation kernels ava_get_spec_batch itself launches, reading their
 * coefficients from the cache: the two paths give the same bits.
 *   audio ... file_len    as ava_get_spec_batch; `files` files
 *   template_dur, fs      the motif is the slice [0, min(len, round(template_dur fs))) of each file; a file with fewer
 *                         than nperseg samples in it yields zeros (utils.py:68-69)
 *   nperseg, noverlap, window, scale, remove_dc     as ava_get_spec_batch (64 <= nperseg <= 2048)
 *   fmin, fmax            smallest / largest target frequency: the cache keeps the bins between them (+- 2)
 *   cache, cache_bytes    device buffer of ava_warp_cache_bytes(...) bytes: per file the frame count, the frame times
 *                         and log(|X| + 1e-12) as [file][bin][frame] float64 (frames padded to a multiple of 16), i.e.
 *                         files x bins x frames x 8 bytes
 *   ws, ws_bytes          scratch of ava_warp_cache_workspace_bytes(...) (build) /
 *                         ava_warp_windows_workspace_bytes(n, F, T, normalize) (windows; needed with normalize only)
 *   file_idx [n], target_times [n][T], target_freqs [F]    device; target times may be non-uniform and may lie
 *                         outside [0, template_dur] (interp2d's fill rule applies); T <= 512
 *   spec_min ... q_gamma  as ava_get_spec_batch;  out [n][F][T] fp32
 * ava_warp_windows must be given the files, template_dur, fs, nperseg, noverlap, fmin, fmax the cache was built with.
 * ava_warp_cache_layout: where things are in a cache of that geometry, out = {maxframes, fstride (doubles from one bin
 * row to the next), k0 (first cached bin), nb (cached bins), off_ftimes, off_logmag}; the offsets are bytes from the
 * first 256-byte boundary at or after `cache`: int32 nframes[files] there, double ftimes[files][maxframes] at off_ftimes,
 * double logmag[files][nb][fstride] at off_logmag, so that
 * ava_warp_cache_bytes(...) == 256 + off_logmag + files * nb * fstride * 8.  AVA_EINVAL where ava_warp_cache_bytes is 0.
 * AVA_EINVAL before any launch for null pointers, files <= 0, template_dur <= 0, an unsupported nperseg or T;
 * AVA_EWORKSPACE for a cache or scratch that is too small.  A file index outside [0, files) gives a window of NaNs.
 *
 * ava_warp_band_spec: the inputs of the warp fit (ava/models/utils.py:337-418, _get_spec for every file): ava_tpl_spec
 * with the divisor handed in, S = clip((log(|X| + 1e-9) - spec_min) / divisor, 0, 1), where the reference's divisor is
 * spec_max_val - spec_min_val + 1e-9 (computed by the caller).  nperseg a power of two in 64..2048. */
size_t ava_warp_cache_bytes(int files, double template_dur, double fs, int nperseg, int noverlap, double fmin,
                            double fmax);
int ava_warp_cache_layout(int files, double template_dur, double fs, int nperseg, int noverlap, double fmin, double fmax,
                          int64_t out[6]);
size_t ava_warp_cache_workspace_bytes(int files, double template_dur, double fs, int nperseg, int noverlap);
int ava_warp_cache_build(const void* audio, int audio_dtype, const int64_t* file_off, const int64_t* file_len, int files,
                         double template_dur, double fs, int nperseg, int noverlap, const double* window, double scale,
                         double fmin, double fmax, int remove_dc, void* cache, size_t cache_bytes, void* ws,
                         size_t ws_bytes, ava_stream_t s);
size_t ava_warp_windows_workspace_bytes(int n, int F, int T, int normalize);
int ava_warp_windows(const void* cache, size_t cache_bytes, int files, double template_dur, double fs, int nperseg,
                     int noverlap, double fmin, double fmax, const int32_t* file_idx, const double* target_times, int n,
                     const double* target_freqs, int F, int T, double spec_min, double spec_max, double fill_value,
                     int normalize, int q_lo, double q_gamma, float* out, void* ws, size_t ws_bytes, ava_stream_t s);
int ava_warp_band_spec(const void* audio, int audio_dtype, const int64_t* file_off, const int64_t* file_len,
                       const int64_t* frame_off, int files, int64_t frames, int nperseg, int noverlap,
                       const double* window, double scale, int k0, int k1, double spec_min, double divisor, double* spec,
                       double* frame_sum, ava_stream_t s);

/* ---- the shift-and-slope time-warp fit ---------------------------------------------
 * ava/preprocessing/warping.py: apply_warp (:25-50), align_specs (:53-145) and its two objectives (:148-163).
 * spec / dtype: [N][F][T] contiguous on the device, 0 = float32, 1 = float64; 2 <= T <= ava_warpfit_max_t() (512: the
 * loss kernel keeps a candidate block's column tables and a set of rows in LDS); N, F >= 1.  All arithmetic is fp64 and
 * no kernel uses atomics: every result is bit-reproducible.  Linear interpolation is scipy's interp1d on the grid
 * 0 .. T-1, operation for operation: value = (y[lo+1] - y[lo]) * (p - lo) + y[lo] with lo = clip(ceil(p), 1, T-1) - 1,
 * nothing fused; p < 0 gives y[0], p > T-1 gives y[T-1], p == T-1 reads columns T-2 and T-1.
 *
 * ava_warpfit_apply: out[n][f][j] = interp(spec[n][f][:])(shift_n + slope_n j), out of spec's dtype.
 *   params [N][2] float64 = (shift, slope).
 * ava_warpfit_mean: target [F][T] float64 = the sum over n = 0, 1, ... in that order, divided by N.
 * ava_warpfit_candidates: cand [N][C][2] = (shift, log slope), C = (2 ks + 1)(2 kl + 1), around x [N][2]: candidate
 *   c = a (2 kl + 1) + b with the offsets oa, ob = 0, -1, +1, -2, +2, ... of a and b, so candidate 0 is x itself;
 *   log slope = x1 + ob hl and shift = x0 + oa hs - (exp(log slope) - exp(x1)) (T - 1) / 2 (the warp pivots about the
 *   middle column).  0 <= ks, kl <= 31, C <= 4096, hs, hl >= 0.
 * ava_warpfit_loss: loss [N][C] float64 = sum_{f,j} (interp(spec[n][f][:])(shift + exp(log slope) j) - target[f][j])^2
 *   + shift_lambda shift^2 + slope_lambda (log slope)^2 for every candidate of cand [N][C][2].  slope_lambda = +inf:
 *   the slope is 1 whatever the candidate says and the slope term is dropped (_get_shift_objective).  1 <= C <= 4096.
 * ava_warpfit_argmin: best [N] int32 = the candidate of least loss; equal losses resolve to the lowest index, NaN never
 *   wins, a motif whose losses are all NaN gets 0.  x [N][2] (needs cand) and best_loss [N] receive that candidate's
 *   parameters and loss when not null.
 *
 * All return AVA_EINVAL before any launch for null pointers, an unknown dtype, N, F or C < 1, T < 2 or T over the cap,
 * a NaN lambda or a grid outside the limits above. */
int ava_warpfit_max_t(void);
int ava_warpfit_apply(const void* spec, int dtype, int N, int F, int T, const double* params, void* out, ava_stream_t s);
int ava_warpfit_mean(const void* spec, int dtype, int N, int F, int T, double* target, ava_stream_t s);
int ava_warpfit_candidates(const double* x, int N, int T, int ks, int kl, double hs, double hl, double* cand,
                           ava_stream_t s);
int ava_warpfit_loss(const void* spec, int dtype, int N, int F, int T, const double* target, const double* cand, int C,
                     double shift_lambda, double slope_lambda, double* loss, ava_stream_t s);
int ava_warpfit_argmin(const double* loss, const double* cand, int N, int C, int32_t* best, double* x, double* best_loss,
                       ava_stream_t s);

/* ---- the piecewise-linear time-warp fit --------------------------------------------
 * The fit above with K = n_knots + 2 knots per motif, 2 <= K <= ava_warpfit_max_knots() (16), T - 1 >= 2 (K - 1).
 * knots / u / a candidate: K float64, u_k = the source position (time bins) template column t_k = k (T-1) / (K-1) maps
 * to.  Column j lies in segment k = min(j (K-1) / (T-1), K-2) (integer division) and reads the source at
 * p(j) = u_k + s_k (j - t_k), s_k = (u_{k+1} - u_k) / (t_{k+1} - t_k), nothing fused; interpolation as above.  K = 2 is
 * the warp above with shift = u_0, slope = s_0.
 *
 * ava_warpfit_pl_apply: out[n][f][j] = interp(spec[n][f][:])(p_n(j)) for knots [N][K], out of spec's dtype.
 * ava_warpfit_pl_candidates: cand [N][C][K], C = 2 ks + 1, around u [N][K]: candidate c moves knot `axis` (axis = -1:
 *   every knot) by o h, o = 0, -1, +1, -2, +2, ..., so candidate 0 is u itself.  -1 <= axis < K, 0 <= ks <= 31, h >= 0.
 * ava_warpfit_pl_loss: loss [N][C] float64 = sum_{f,j} (interp(spec[n][f][:])(p(j)) - target[f][j])^2
 *   + shift_lambda u_0^2 + slope_lambda (sum_k (log s_k)^2) / (K - 1) for every candidate of cand [N][C][K]; +inf for a
 *   candidate with some s_k <= 0 (knots out of order).  slope_lambda = +inf: p(j) = u_0 + j whatever the other knots say,
 *   the slope term is dropped and no candidate is out of order.  1 <= C <= 4096.  Same kernel structure, LDS and
 *   summation order as ava_warpfit_loss.
 * ava_warpfit_pl_argmin: ava_warpfit_argmin for candidates of K parameters: u [N][K] receives the best candidate.
 *   +inf loses to every finite loss.
 *
 * All return AVA_EINVAL before any launch on the conditions of the entry points above, or for K outside the limits. */
int ava_warpfit_max_knots(void);
int ava_warpfit_pl_apply(const void* spec, int dtype, int N, int F, int T, const double* knots, int K, void* out,
                         ava_stream_t s);
int ava_warpfit_pl_candidates(const double* u, int N, int K, int axis, int ks, double h, double* cand, ava_stream_t s);
int ava_warpfit_pl_loss(const void* spec, int dtype, int N, int F, int T, const double* target, const double* cand, int C,
                        int K, double shift_lambda, double slope_lambda, double* loss, ava_stream_t s);
int ava_warpfit_pl_argmin(const double* loss, const double* cand, int N, int C, int K, int32_t* best, double* u,
                          double* best_loss, ava_stream_t s);

/* ---- the grouped time-warp fits ------------------------------------------------------
 * Many fit problems ("groups") over one spec [N][F][T], advanced together by the kernels above.  A group is a sorted
 * list of source rows (motifs), a sorted list of bins and its own two lambdas.  The plan, int32 on the device:
 *   row_src [V], row_group [V]   virtual row v is motif row_src[v] as group row_group[v] sees it; a group's rows are
 *                                contiguous, in rising source order
 *   group_row_off [G+1]          group g owns the virtual rows group_row_off[g] .. group_row_off[g+1] - 1
 *   bin_off [G+1], bins [sum F_g] group g owns bins[bin_off[g] .. bin_off[g+1] - 1], F_g of them, rising
 *   targets                      float64, group g's [F_g][T] by list position at targets + bin_off[g] T
 *   shift_lambda [G], slope_lambda [G]   float64
 * ava_warpfit_candidates, _pl_candidates, _argmin and _pl_argmin serve the V virtual rows as they are (N = V).
 *
 * ava_warpfit_group_loss / ava_warpfit_group_pl_loss: loss [V][C] for cand [V][C][2] / [V][C][K]: for every virtual row
 *   bit for bit what ava_warpfit_loss / ava_warpfit_pl_loss return on the gathered tensor spec[rows_g][:, bins_g] with
 *   the group's target and lambdas: the bins are staged through the list, in list order, the sums are the plain
 *   kernel's.  fixed_slope (0 / 1) is one flag for the launch: the shift objective, slope_lambda is not read.  raw = 1:
 *   the sum of squared differences of the unwarped rows from the target, no penalty; cand and the lambdas are not read
 *   and may be null.
 * ava_warpfit_group_mean / ava_warpfit_group_pl_mean: targets = for every group the mean over its rows, in rising
 *   order, of the values ava_warpfit_apply / ava_warpfit_pl_apply would store under params [V][2] = (shift, slope) /
 *   knots [V][K] (rounded to spec's dtype first), bit for bit ava_warpfit_mean of that output on the gathered tensor,
 *   without storing it.  raw = 1: the mean of the unwarped rows; params may be null.  max_bins: the largest F_g.
 *
 * The caller keeps every index of the plan in range and every list non-empty (ava_amd.warp_fit checks them on the
 * host); a row or bin out of range reads nothing and yields NaN or leaves the loss unwritten.  AVA_EINVAL before any
 * launch for null pointers, an unknown dtype, sizes < 1, T, C or K outside the caps above, or a flag that is not 0 / 1. */
int ava_warpfit_group_loss(const void* spec, int dtype, int N, int F, int T, const int32_t* row_src, const int32_t* row_group,
                           const int32_t* bin_off, const int32_t* bins, int V, const double* targets, const double* cand,
                           int C, const double* shift_lambda, const double* slope_lambda, int fixed_slope, int raw,
                           double* loss, ava_stream_t s);
int ava_warpfit_group_pl_loss(const void* spec, int dtype, int N, int F, int T, const int32_t* row_src,
                              const int32_t* row_group, const int32_t* bin_off, const int32_t* bins, int V,
                              const double* targets, const double* cand, int C, int K, const double* shift_lambda,
                              const double* slope_lambda, int fixed_slope, int raw, double* loss, ava_stream_t s);
int ava_warpfit_group_mean(const void* spec, int dtype, int N, int F, int T, const int32_t* row_src,
                           const int32_t* group_row_off, const int32_t* bin_off, const int32_t* bins, int G, int max_bins,
                           const double* params, int raw, double* targets, ava_stream_t s);
int ava_warpfit_group_pl_mean(const void* spec, int dtype, int N, int F, int T, const int32_t* row_src,
                              const int32_t* group_row_off, const int32_t* bin_off, const int32_t* bins, int G, int max_bins,
                              const double* knots, int K, int raw, double* targets, ava_stream_t s);

/* ---- the integer-shift time-warp fit -------------------------------------------------
 * The alignment of ava/segmenting/template_segmentation.py:segment_sylls_from_songs (:531-539), this project's own model
 * in place of affinewarp's ShiftWarping (ava_amd/shift_fit.py states it).  x / dtype: [K][F][T] contiguous on the
 * device, 0 = float32, 1 = float64; 3 <= T <= ava_shiftfit_max_t() (2048), F T < 2^30.  All arithmetic is fp64.
 * Template column t lies at raw column t + s_k, the end columns held.  Lags are ordered lag_c = 0, -1, +1, -2, +2, ...,
 * -L, +L (c = 0 .. 2 L).
 *
 * ava_shiftfit_workspace_bytes: device scratch ava_shiftfit_template needs (0 for an unsupported shape).
 * ava_shiftfit_template: mbar [F][T] (may be NULL) = sum_k x[k][f][clip(t + s_k, 0, T-1)] / K, summed in chunks of 128
 *   renditions (within a chunk in rising k, then the chunks in rising order: the bits do not depend on the grid), and
 *   tmpl [F][T] = the solution of A tmpl[f][:] = mbar[f][:], A = (1 + l2 / K) I + smoothness D2^T D2 (D2: the second
 *   differences (1, -2, 1)), by a banded LDL^T.  shifts [K] int32; smoothness, l2 >= 0 and finite; K <= 65535 * 128.
 * ava_shiftfit_loss: loss [K][2 L + 1] float64 = sum_{f,t} (x[k][f][clip(t + lag_c, 0, T-1)] - tmpl[f][t])^2 / (F T),
 *   0 <= L <= T - 1.  Every term is one rounded subtraction and one rounded multiplication; the sum runs in a fixed
 *   order (csrc/shift_fit.hip), no atomics: two calls give the same bits.
 * ava_shiftfit_argmin: shifts [K] int32 = the lag of least loss; equal losses resolve to the lowest c (so 0 beats -1
 *   beats +1 ...), NaN never wins (all NaN: shift 0).  best_loss [K] (may be NULL) = that loss.
 * ava_shiftfit_apply: out[k][f][t] = x[k][f][clip(t + s_k, 0, T-1)], out of x's dtype: exact copies.
 *
 * All return AVA_EINVAL before any launch for null pointers, an unknown dtype, K or F < 1, T outside the limits, L
 * outside its range or a negative, infinite or NaN penalty; ava_shiftfit_template AVA_EWORKSPACE for too little scratch. */
int ava_shiftfit_max_t(void);
size_t ava_shiftfit_workspace_bytes(int K, int F, int T);
int ava_shiftfit_template(const void* x, int dtype, int K, int F, int T, const int32_t* shifts, double smoothness, double l2,
                          double* mbar, double* tmpl, void* ws, size_t ws_bytes, ava_stream_t s);
int ava_shiftfit_loss(const void* x, int dtype, int K, int F, int T, const double* tmpl, int L, double* loss, ava_stream_t s);
int ava_shiftfit_argmin(const double* loss, int K, int L, int32_t* shifts, double* best_loss, ava_stream_t s);
int ava_shiftfit_apply(const void* x, int dtype, int K, int F, int T, const int32_t* shifts, void* out, ava_stream_t s);

/* ---- exact 1-nearest-neighbour search ------------------------------------------------
 * The searches of ava/plotting/shotgun_movie.py:shotgun_movie_DC: NearestNeighbors(n_neighbors=1,
 * metric='correlation') over spectrograms (:148-158) and argmin of scipy's euclidean over latent means (:126-133).
 *
 * ava_nn_workspace_bytes: device scratch ava_nn_argmin needs (0 for an unsupported shape or metric).
 *
 * ava_nn_argmin: for each of nq query rows the nearest of nr reference rows.
 *   queries, q_dtype      [nq][d] row-major on the device; 0 = float32, 1 = float64
 *   refs, r_dtype         [nr][d] likewise
 *   metric                0 = correlation, 1 - (q - mean q).(r - mean r) / (|q - mean q| |r - mean r|), the cosine
 *                         clipped to [-1, 1] as scipy clips it; 1 = euclidean, sqrt(sum (q - r)^2)
 *   out_idx, out_dist     [nq] int64 index of the nearest reference and its distance (float64), device
 * nq, nr >= 1, 1 <= d <= 65536.  All arithmetic is fp64.  Equal distances resolve to the lowest index.  Correlation: a
 * zero-variance row gives NaN distances, NaN loses to any number, and a query whose distances are all NaN gets index
 * 0 and NaN.  Euclidean: NaN wins and the first NaN is taken (np.argmin).  The results are bit-reproducible.
 *
 * ava_nn_merge: fold the result of a later chunk of references into a running result: (idx[q] + offset, dist[q])
 * replaces (best_idx[q], best_dist[q]) when it is better under the same order, so the earlier chunk wins ties.
 *
 * Both return AVA_EINVAL before any launch for null pointers, an unknown dtype or metric or an unsupported shape;
 * ava_nn_argmin returns AVA_EWORKSPACE for a workspace that is too small. */
size_t ava_nn_workspace_bytes(int nq, int nr, int d, int metric);
int ava_nn_argmin(const void* queries, int q_dtype, int nq, const void* refs, int r_dtype, int nr, int d, int metric,
                  int64_t* out_idx, double* out_dist, void* ws, size_t ws_bytes, ava_stream_t s);
int ava_nn_merge(int64_t* best_idx, double* best_dist, const int64_t* idx, const double* dist, int nq, int64_t offset,
                 int metric, ava_stream_t s);

/* ---- UMAP and PCA projections of latent means (DataContainer 'latent_mean_umap' / 'latent_mean_pca') --------------
 * ava/data/data_container.py:514-551.  All arithmetic is fp64, nothing uses atomics, and every result is
 * bit-reproducible and independent of the launch shape.  x / dtype: [n][d] row-major on the device, 0 = float32,
 * 1 = float64.
 *
 * ava_pj_knn: rows [q0, q0 + nq) of the exact euclidean k-nearest-neighbour table of x among its own rows:
 *   out_idx [nq][k] int64, out_dist [nq][k] float64 (device).  Column 0 is the row itself at distance 0; columns
 *   1 .. k-1 are the nearest other rows ordered by (distance, index).  1 <= k <= min(64, n), 1 <= d <= 65536.
 *
 * ava_pj_smooth: umap's smooth_knn_dist (64 bisection steps, tolerance 1e-5, floor 1e-3 x mean distance) and
 *   compute_membership_strengths on a [n][k] kNN table: sigma [n], rho [n], w [n][k] (0 for the row itself);
 *   mean_all [1] receives the mean of the whole distance table.
 *
 * ava_pj_layout: epochs [e0, e1) of n_epochs of the synchronous SGD layout of y [n][2] (in / out; y_tmp the same size)
 *   over the symmetric CSR graph indptr [n + 1] int64, col [nnz] int32 with per-edge eps (epochs per sample), epn
 *   (epochs per negative sample) and the two counters next_s / next_n (in / out).  The learning rate of epoch e is
 *   learning_rate for e = 0 and learning_rate (1 - (e - 1) / n_epochs) after; negative samples come from the
 *   splitmix64 hash of ((e nnz + edge) 16 + p, salt).  flag [1] int is set to 1 if an edge needed more than 16
 *   negative samples in one epoch (they are clamped to 16).  All epochs are enqueued without a host synchronisation.
 *
 * The out-of-sample half (umap's transform; nothing below writes the training data):
 * ava_pj_knn_query: rows [q0, q0 + nq) of the table of the k nearest of the n reference rows x [n][d] of each of the m
 *   query rows q [m][d] (one dtype for both), ordered by (distance, index), no row excluded; the distance arithmetic
 *   is that of ava_pj_knn.  1 <= k <= min(64, n), 1 <= d <= 65536.
 * ava_pj_row_stats: stats [n][2] float64 (device): the fp64 mean and the centred sum of squares of every row of x, each a
 *   fixed-order two-stage sum (csrc/corr_tile.h).  1 <= d <= 65536.
 * ava_pj_knn_corr / ava_pj_knn_corr_query: ava_pj_knn / ava_pj_knn_query under umap-learn's correlation distance, with
 *   the operands' statistics from ava_pj_row_stats (xstat [n][2], qstat [m][2]): dist = 1 - dot / sqrt(ss_q ss_r), the
 *   dot product of the centred rows on the fp64 matrix cores, the cosine clipped to [-1, 1]; 0 when both rows have a
 *   centred sum of squares of exactly 0, 1 when exactly one has.  Every distance is finite.  Same table layout, order
 *   (distance, index), modes and limits; the dot products take k in one fixed order, so the table does not depend on
 *   q0 / nq, and a pair of rows gets the bits ava_nn_argmin's correlation gives it.
 * ava_pj_smooth_bipartite: ava_pj_smooth for a table whose columns index another set than its rows: no weight is
 *   zeroed for idx == row.
 * ava_pj_transform_init: wn [m][k] = w / (row sum, left to right; a row of sum 0 stays 0) and y0 [m][2] =
 *   sum_s wn[i][s] emb[idx[i][s]] in slot order; emb [n_train][2] float64.  idx must lie in [0, n_train).
 * ava_pj_transform_layout: epochs [0, epochs) of n_epochs of the layout of the new points y [m][2] (in / out) against
 *   the fixed emb, in one launch, a thread per row moving edge by edge: a due slot pulls y towards its neighbour once,
 *   then pushes it from min(16, due) negative samples emb[min(floor(u n_train), n_train - 1)], u the splitmix64 hash
 *   of (((e m + i) k + s) 16 + p, salt), each from the already moved y (a sample at distance 0 moves nothing).
 *   eps / epn [k][m] slot-major (eps <= 0: the slot is pruned); the step of epoch e is learning_rate / 4 for e = 0
 *   and (learning_rate / 4) (1 - (e - 1) / n_epochs) after; flag as in ava_pj_layout.
 *
 * ava_pj_gram_workspace_bytes / ava_pj_gram: gram [(d+1)][(d+1)] = [x, 1]^T [x, 1] (so gram[i][d] is the sum of column
 *   i and gram[d][d] = n), summed over fixed row chunks in order.  1 <= d <= 512.
 *
 * ava_pj_project: out [n][nc] = x V^T - muv, V [nc][d], muv [nc] (device, float64).
 *
 * All return AVA_EINVAL before any launch for null pointers, an unknown dtype or an unsupported shape;
 * ava_pj_gram returns AVA_EWORKSPACE for a workspace that is too small. */
int ava_pj_knn(const void* x, int dtype, int n, int d, int k, int q0, int nq, int64_t* out_idx, double* out_dist,
               ava_stream_t s);
int ava_pj_smooth(const double* dist, const int64_t* idx, int n, int k, double local_connectivity, double* mean_all,
                  double* sigma, double* rho, double* w, ava_stream_t s);
int ava_pj_layout(double* y, double* y_tmp, const int64_t* indptr, const int* col, const double* eps,
                  const double* epn, double* next_s, double* next_n, int n, int64_t nnz, int e0, int e1, int n_epochs,
                  double learning_rate, double a, double b, double gamma, uint64_t salt, int* flag, ava_stream_t s);
int ava_pj_knn_query(const void* q, const void* x, int dtype, int m, int n, int d, int k, int q0, int nq,
                     int64_t* out_idx, double* out_dist, ava_stream_t s);
int ava_pj_row_stats(const void* x, int dtype, int n, int d, double* stats, ava_stream_t s);
int ava_pj_knn_corr(const void* x, int dtype, const double* xstat, int n, int d, int k, int q0, int nq,
                    int64_t* out_idx, double* out_dist, ava_stream_t s);
int ava_pj_knn_corr_query(const void* q, const void* x, int dtype, const double* qstat, const double* xstat, int m,
                          int n, int d, int k, int q0, int nq, int64_t* out_idx, double* out_dist, ava_stream_t s);
int ava_pj_smooth_bipartite(const double* dist, const int64_t* idx, int n, int k, double local_connectivity,
                            double* mean_all, double* sigma, double* rho, double* w, ava_stream_t s);
int ava_pj_transform_init(const double* w, const int64_t* idx, const double* emb, int m, int k, double* wn, double* y0,
                          ava_stream_t s);
int ava_pj_transform_layout(double* y, const double* emb, const int64_t* idx, const double* eps, const double* epn,
                            int m, int k, int n_train, int epochs, int n_epochs, double learning_rate, double a,
                            double b, double gamma, uint64_t salt, int* flag, ava_stream_t s);
size_t ava_pj_gram_workspace_bytes(int n, int d);
int ava_pj_gram(const void* x, int dtype, int n, int d, double* gram, void* ws, size_t ws_bytes, ava_stream_t s);
int ava_pj_project(const void* x, int dtype, int n, int d, const double* V, const double* muv, int nc, double* out,
                   ava_stream_t s);

/* ---- Exact t-SNE (row f19; sklearn 1.7 TSNE(method='exact', n_components=2); csrc/tsne.hip) -------------------------
 * The N x N matrix m (squared distances, then joint probabilities) is float64 row-major on the device with a row
 * stride ld >= n, ld even, on a 16-byte boundary; 2 <= n <= ava_ts_max_n() = 32768.  Everything is fp64 and free of
 * atomics: the same inputs give the same bits on every run.  ws: ava_ts_workspace_bytes(n, col_chunks) bytes.
 *
 * ava_ts_col_chunks: the number of column chunks the descent kernels split the pairs into by default, a function of
 *   n alone (0 for an unsupported n); col_chunks <= 0 in the calls below means this value, at most 64 may be passed.
 * ava_ts_sqdist: out[i][j] = |x_i - x_j|^2 of the rows x [n][d] (dtype 0 = float32, 1 = float64; 1 <= d <= 65536)
 *   with the bits of ava_pair_sqdist, rounded to the nearest float32 (and stored as float64) when round_f32 != 0.
 * ava_ts_square: out[i][j] = float32(dist[i][j]^2) of a contiguous float64 [n][n] distance matrix.
 * ava_ts_joint: in place, the squared distances become sklearn's joint probabilities P (_joint_probabilities with
 *   _binary_search_perplexity; symmetric, zero diagonal, every other entry >= DBL_EPSILON).  0 < perplexity < n.
 * ava_ts_kl_gradient: stats[0] = KL(e P || Q), stats[1] = |grad|_2 and grad [n][2] = dKL/dy at y [n][2] (sklearn's
 *   _kl_divergence with P scaled by the exaggeration e).
 * ava_ts_descend: n_iters iterations of sklearn's _gradient_descent on y, update, gains [n][2] (in / out), enqueued
 *   without a host synchronisation; stats [n_iters][2] receives every iteration's {KL, |grad gains|_2}, the KL of
 *   all but the last as NaN (not computed, like sklearn's compute_error=False: it costs more than the rest of the pass).
 *
 * All return AVA_EINVAL before any launch for null or misaligned pointers or an unsupported shape, AVA_EWORKSPACE for
 * a workspace that is too small. */
int ava_ts_max_n(void);
int ava_ts_col_chunks(int n);
size_t ava_ts_workspace_bytes(int n, int col_chunks);
int ava_ts_sqdist(const void* x, int dtype, int n, int d, int round_f32, double* out, int ld, ava_stream_t s);
int ava_ts_square(const double* dist, int n, double* out, int ld, ava_stream_t s);
int ava_ts_joint(double* p, int ld, int n, double perplexity, void* ws, size_t ws_bytes, ava_stream_t s);
int ava_ts_kl_gradient(const double* y, const double* p, int ld, int n, double exaggeration, int col_chunks,
                       double* grad, double* stats, void* ws, size_t ws_bytes, ava_stream_t s);
int ava_ts_descend(double* y, double* update, double* gains, const double* p, int ld, int n, int n_iters,
                   double momentum, double lr, double exaggeration, int col_chunks, double* stats, void* ws,
                   size_t ws_bytes, ava_stream_t s);

/* ---- Gaussian mixture models (row f20; sklearn 1.7 GaussianMixture, 'full' and 'diag'; csrc/mixture.hip) -----------
 * x / dtype: [n][d] row-major on the device, 0 = float32, 1 = float64.  cov_type: 0 = 'full', 1 = 'diag'.  All other
 * arrays are float64 on the device: weights [k], means [k][d], cov and prec_chol [k][d][d] ('full'; prec_chol is
 * sklearn's precisions_cholesky_, upper triangular) or [k][d] ('diag'), log_det [k] = sum log diag prec_chol,
 * log_prob_norm [n], log_resp and resp [n][k].  1 <= d <= ava_gm_max_d() = 128, 1 <= k <= ava_gm_max_k() = 64,
 * k <= n.  Everything is fp64 in fixed orders (the contract at the head of mixture.hip): the same inputs give the same
 * bits on every run.  Partial sums are taken over chunks of ava_gm_chunk_rows() = 2048 rows, a constant.
 * ws: ava_gm_workspace_bytes(n, d, k, cov_type) bytes (0 for an unsupported shape).
 *
 * ava_gm_e_step: sklearn's _estimate_log_prob_resp at the given parameters, and resp = exp(log_resp).
 * ava_gm_means:  nk [k] = sum_n resp + 10 DBL_EPSILON, means = sum_n resp x / nk, weights = nk / n normalised
 *   (ws of cov_type 1).
 * ava_gm_m_step: sklearn's _m_step from resp: ava_gm_means, then cov = sum_n resp (x - mean)(x - mean)^T / nk +
 *   reg_covar I (exactly symmetric; 'diag': the diagonal), its Cholesky factor L, prec_chol = (L^-1)^T and log_det.
 *   status [1] int is set to 1 when a covariance is not positive definite (nothing is read or written out of bounds;
 *   prec_chol and log_det of that component are then undefined); the caller clears it.
 * ava_gm_fit: iterations [it0, it0 + n_iters) of sklearn's EM loop (E-step, M-step, |lower bound - previous| < tol),
 *   enqueued without a host synchronisation; the parameters advance in place.  lower_bounds [>= it0 + n_iters] receives
 *   every iteration's bound; ctl [>= 3 + it0 + n_iters] int: ctl[0] the status word of ava_gm_m_step, ctl[1] the number
 *   of iterations that ran, ctl[2 + i] whether the loop had stopped before iteration i (ctl[2 + it0 + n_iters] after
 *   the call: whether it has stopped).  The caller zeroes ctl before iteration 0.  Once the loop has stopped, or
 *   ctl[0] is set, every later launch returns at once, so the parameters are those of the stopping iteration.
 *   log_prob_norm, log_resp and resp are scratch and hold the last E-step that ran.
 * ava_gm_onehot: resp [n][k] = (labels[i] == j); changed [1] int += the number of rows with labels[i] != prev[i];
 *   prev = labels (int64, device).
 *
 * All return AVA_EINVAL before any launch for null pointers, an unknown dtype or cov_type, negative tol or reg_covar or
 * an unsupported shape, AVA_EWORKSPACE for a workspace that is too small. */
int ava_gm_max_d(void);
int ava_gm_max_k(void);
int ava_gm_chunk_rows(void);
size_t ava_gm_workspace_bytes(int n, int d, int k, int cov_type);
int ava_gm_e_step(const void* x, int dtype, int n, int d, int k, int cov_type, const double* weights,
                  const double* means, const double* prec_chol, const double* log_det, double* log_prob_norm,
                  double* log_resp, double* resp, ava_stream_t s);
int ava_gm_means(const void* x, int dtype, int n, int d, int k, const double* resp, double* weights, double* means,
                 double* nk, void* ws, size_t ws_bytes, ava_stream_t s);
int ava_gm_m_step(const void* x, int dtype, int n, int d, int k, int cov_type, const double* resp, double reg_covar,
                  double* weights, double* means, double* cov, double* prec_chol, double* log_det, int* status,
                  void* ws, size_t ws_bytes, ava_stream_t s);
int ava_gm_fit(const void* x, int dtype, int n, int d, int k, int cov_type, double* weights, double* means,
               double* cov, double* prec_chol, double* log_det, double tol, double reg_covar, int it0, int n_iters,
               double* lower_bounds, int* ctl, double* log_prob_norm, double* log_resp, double* resp, void* ws,
               size_t ws_bytes, ava_stream_t s);
int ava_gm_onehot(const int64_t* labels, int64_t* prev, int n, int k, double* resp, int* changed, ava_stream_t s);

/* ---- Silhouette and cluster-validity sums (row f21; sklearn 1.7 metrics/cluster/_unsupervised.py; csrc/silhouette.hip)
 * x / dtype: [n][d] row-major on the device, 0 = float32, 1 = float64, d >= 1.  The labels are encoded by the caller as
 * 0 .. k - 1 with 2 <= k <= min(n - 1, ava_sil_max_k() = 1024).  order [n] int64: the stable argsort of the encoded
 * labels ("sorted row r" is the caller's row order[r]); off [k + 1] int64: cluster j owns the sorted rows
 * [off[j], off[j + 1]).  Both on the device; entries out of range are clamped or skipped, never followed out of bounds.
 * Everything is fp64 in fixed orders (the contract at the head of silhouette.hip): a cluster's columns are added in
 * chunks of ava_sil_chunk_cols() = 2048 counted from the cluster's first column, so sums [.][j] depends on the rows of
 * cluster j and on the row itself only.  ws: ava_sil_workspace_bytes(n, d, k) bytes (0 for an unsupported shape; the
 * rows in cluster order and the chunk partials; the size for d serves every smaller d).
 *
 * ava_sil_cluster_sums: sums [n][k], row r = sorted row r: sums[r][j] = sum over the rows c of cluster j of
 *   sqrt(sum_f (x_rf - x_cf)^2), direct differences, f ascending (the bits of ava_pair_sqdist), one fp64 sqrt.
 * ava_sil_cluster_sums_pre: the same sums from dist [n][n] (dtype as x), distances in the caller's row order.
 * ava_sil_finish: per sorted row r of cluster l: a = sums[r][l] / (n_l - 1), b = min_{j != l} sums[r][j] / n_j,
 *   s = (b - a) / max(a, b), 0 where that is NaN; sil, a, b [n] in the caller's row order; score [1] = mean of sil
 *   over chunks of 2048 rows added ascending.  ws: at least ava_sil_workspace_bytes(n, 1, k).
 * ava_sil_centroid_stats: labels [n] int64 encoded labels in the caller's order, means [k][d] (ava_gm_onehot +
 *   ava_gm_means); sum_dist [k] = sum over the rows of cluster j of ||x - means[j]||, sum_sq [k] of its square; chunks
 *   of 2048 rows ascending.  d <= ava_gm_max_d(), k <= ava_gm_max_k().
 *
 * All return AVA_EINVAL before any launch for null pointers, an unknown dtype or an unsupported shape, AVA_EWORKSPACE
 * for a workspace that is too small. */
int ava_sil_max_k(void);
int ava_sil_chunk_cols(void);
size_t ava_sil_workspace_bytes(int n, int d, int k);
int ava_sil_cluster_sums(const void* x, int dtype, int n, int d, int k, const int64_t* order, const int64_t* off,
                         double* sums, void* ws, size_t ws_bytes, ava_stream_t s);
int ava_sil_cluster_sums_pre(const void* dist, int dtype, int n, int k, const int64_t* order, const int64_t* off,
                             double* sums, ava_stream_t s);
int ava_sil_finish(const double* sums, int n, int k, const int64_t* order, const int64_t* off, double* sil, double* a,
                   double* b, double* score, void* ws, size_t ws_bytes, ava_stream_t s);
int ava_sil_centroid_stats(const void* x, int dtype, int n, int d, int k, const int64_t* labels, const double* means,
                           double* sum_dist, double* sum_sq, void* ws, size_t ws_bytes, ava_stream_t s);

/* ---- DBSCAN (row f22; sklearn 1.7 cluster/_dbscan.py and _dbscan_inner.pyx; csrc/dbscan.hip) -------------------------
 * x / dtype: [n][d] row-major on the device, 0 = float32, 1 = float64, 1 <= d <= 65536, 1 <= n <= 2^21.  The _pre forms
 * take dist [n][n] (dtype as x), a SYMMETRIC matrix of distances, in its place.  eps [n_eps]: HOST array of the radii,
 * each positive and finite, 1 <= n_eps <= ava_db_max_eps() = 8; a pass forms every pair's distance once and compares it
 * n_eps times, and all per-radius arrays are laid out [n_eps][n].  A pair is within radius e when d2 <= eps[e] * eps[e]
 * (the product rounded once in fp64, d2 the direct-difference sum of ava_pair_sqdist, no square root), or when
 * (double)dist[i][j] <= eps[e], i < j.  Only integer atomics whose outcome does not depend on their order are used: the
 * same inputs give the same output on every run.  ws: ava_db_workspace_bytes(n, d, n_eps) bytes (0 for an unsupported
 * shape).
 *
 * ava_db_counts: counts [n_eps][n] int (device) = the number of rows within the radius of each row, itself included.
 * ava_db_union: row i is a core row of radius e when counts[e][i] >= min_samples (>= 1).  The connected components of
 *   the core rows under "within the radius" by a lock-free union-find that hooks the larger root under the smaller;
 *   leaves in ws every core row's root = the smallest row of its component.
 * ava_db_assign: after ava_db_union on the same ws and arguments: core [n_eps][n] bytes (1 = core row), labels
 *   [n_eps][n] int64 and n_clusters [n_eps] int (all device).  The components are numbered 0, 1, .. in ascending order
 *   of their smallest row; a non-core row with core rows within the radius takes the smallest cluster number among
 *   them; every other row is -1.
 * ava_db_labels: ava_db_union, then ava_db_assign.
 *
 * All return AVA_EINVAL before any HIP call for null pointers, an unknown dtype, an unsupported shape, a bad radius or
 * min_samples < 1, AVA_EWORKSPACE for a workspace that is too small. */
int ava_db_max_eps(void);
size_t ava_db_workspace_bytes(int n, int d, int n_eps);
int ava_db_counts(const void* x, int dtype, int n, int d, const double* eps, int n_eps, int* counts, ava_stream_t s);
int ava_db_counts_pre(const void* dist, int dtype, int n, const double* eps, int n_eps, int* counts, ava_stream_t s);
int ava_db_union(const void* x, int dtype, int n, int d, const double* eps, int n_eps, int min_samples,
                 const int* counts, void* ws, size_t ws_bytes, ava_stream_t s);
int ava_db_union_pre(const void* dist, int dtype, int n, const double* eps, int n_eps, int min_samples,
                     const int* counts, void* ws, size_t ws_bytes, ava_stream_t s);
int ava_db_assign(const void* x, int dtype, int n, int d, const double* eps, int n_eps, int min_samples,
                  const int* counts, unsigned char* core, int64_t* labels, int* n_clusters, void* ws, size_t ws_bytes,
                  ava_stream_t s);
int ava_db_assign_pre(const void* dist, int dtype, int n, const double* eps, int n_eps, int min_samples,
                      const int* counts, unsigned char* core, int64_t* labels, int* n_clusters, void* ws,
                      size_t ws_bytes, ava_stream_t s);
int ava_db_labels(const void* x, int dtype, int n, int d, const double* eps, int n_eps, int min_samples,
                  const int* counts, unsigned char* core, int64_t* labels, int* n_clusters, void* ws, size_t ws_bytes,
                  ava_stream_t s);
int ava_db_labels_pre(const void* dist, int dtype, int n, const double* eps, int n_eps, int min_samples,
                      const int* counts, unsigned char* core, int64_t* labels, int* n_clusters, void* ws,
                      size_t ws_bytes, ava_stream_t s);

/* ---- HDBSCAN (row f23; sklearn 1.7 cluster/_hdbscan: hdbscan.py, _reachability.pyx, _linkage.pyx, _tree.pyx;
 * csrc/hdbscan.hip) ------------------------------------------------------------------------------------------------------
 * x / dtype: [n][d] row-major on the device, 0 = float32, 1 = float64, 1 <= d <= 65536, 2 <= n <= 2^21.  The _pre forms
 * take dist [n][n] (dtype as x), a SYMMETRIC matrix of distances, in its place.  The pair measure m(i, j) is the
 * direct-difference sum d2 of ava_pair_sqdist (no square root) or (double)dist[i][j]; core [n] (device, float64) is the
 * min_samples-th smallest m(i, .), the row itself (as 0) counted first; w(i, j) = max(core[i], core[j], m(i, j)).  Edges
 * are ordered by the key (w, m, min(i, j), max(i, j)), a strict total order: the minimum spanning tree is unique.
 *
 * ava_hd_core: kth [n] int64 (device) = the row of each row's min_samples-th neighbour (column min_samples - 1 of
 *   ava_pj_knn's table); core[i] = d2(i, kth[i]) in the fma order of the distance tile.
 * ava_hd_core_pre: core[i] = the k-th smallest of row i of dist, its diagonal entry read as 0; 1 <= k <= min(64, n).
 * ava_hd_mst: Boruvka rounds on the device.  ei, ej [n - 1] int, ew, em [n - 1] float64 (device): the n - 1 tree edges
 *   (ei < ej) with their w and m, in NO particular order (sort them by the key).  rounds (HOST int): the rounds taken,
 *   at most ava_hd_max_rounds(n) = ceil(log2 n); rowmin_ms (HOST float [ava_hd_max_rounds(n)], may be NULL): the time
 *   of each round's row-minimum launch, by device events.  The call reads one word per round back and returns with the
 *   stream idle.  AVA_ELAUNCH also when a round leaves more than half of its components (impossible for finite input).
 *   ws: ava_hd_workspace_bytes(n, d) bytes (0 for an unsupported shape; d = 1 for the _pre form).
 * ava_hd_tree: HOST code, no HIP call, every pointer a host pointer.  ei, ej int64 and dist float64 [n - 1]: the tree's
 *   edges in ascending key order with the distances to report (sqrt(w) or w).  sklearn's make_single_linkage,
 *   _condense_tree, _compute_stability, _get_clusters (method 0 = 'eom', 1 = 'leaf'; allow_single_cluster = False,
 *   cluster_selection_epsilon = 0, max_cluster_size = None), _do_labelling and get_probabilities: labels [n] int64
 *   (noise -1, clusters numbered in ascending order of their smallest row), prob [n] float64, *n_clusters, linkage
 *   [n - 1][4] float64 (scipy's format: the cluster of ei, the cluster of ej, the distance, the size).  AVA_EINVAL
 *   for edges that are no spanning tree, a NaN distance, min_cluster_size < 2 or an unknown method.
 *
 * All return AVA_EINVAL before any HIP call for null pointers, an unknown dtype or an unsupported shape, AVA_EWORKSPACE
 * for a workspace that is too small. */
size_t ava_hd_workspace_bytes(int n, int d);
int ava_hd_max_rounds(int n);
int ava_hd_core(const void* x, int dtype, int n, int d, const int64_t* kth, double* core, ava_stream_t s);
int ava_hd_core_pre(const void* dist, int dtype, int n, int k, double* core, ava_stream_t s);
int ava_hd_mst(const void* x, int dtype, int n, int d, const double* core, int* ei, int* ej, double* ew, double* em,
               int* rounds, float* rowmin_ms, void* ws, size_t ws_bytes, ava_stream_t s);
int ava_hd_mst_pre(const void* dist, int dtype, int n, const double* core, int* ei, int* ej, double* ew, double* em,
                   int* rounds, float* rowmin_ms, void* ws, size_t ws_bytes, ava_stream_t s);
int ava_hd_tree(const int64_t* ei, const int64_t* ej, const double* dist, int n, int min_cluster_size, int method,
                int64_t* labels, double* prob, int* n_clusters, double* linkage);

/* ---- cross-validated k-nearest-neighbour prediction (row f24; sklearn 1.7 neighbors/_classification.py, _regression.py,
 * _base.py::_get_weights under cross_val_predict with a PredefinedSplit; csrc/knn_predict.hip) ---------------------------
 * ava_kp_knn_masked: rows [q0, q0 + nq) of the table of the k nearest rows of every row of x [n][d] (dtype 0 = float32,
 *   1 = float64; device) among the rows of OTHER folds: reference r is a candidate of query q unless
 *   fold[r] == fold[q] (fold [n] int, device).  out_idx [nq][k] int64, out_dist [nq][k] float64 (device), ordered by
 *   (distance, index); the distance arithmetic is that of ava_pj_knn, bit for bit.  A row is in its own fold, so it is
 *   never its own neighbour.  1 <= k <= min(64, n), n <= 2^30, 1 <= d <= 65536.  The caller guarantees that every row has k
 *   candidates (n minus the largest fold >= k); a slot without one is written as index -1 at distance 0.
 * The three below read a [nq][kmax] table of that form (kmax <= 64; every index a row of y / Y) and a sweep ks (HOST int
 *   [n_k], 1 <= n_k <= ava_kp_max_sweep() = 16, strictly ascending, 1 <= ks[a] <= kmax): the list for ks[a] is the first
 *   ks[a] slots.  The weight of a slot is 1 (weighted = 0) or 1 / distance (weighted = 1), except in a row whose slot 0
 *   is at distance 0, where it is 1 for the slots at distance 0 and 0 for the others.
 * ava_kp_vote: y [n] int (device): the class codes of the reference rows.  out_pred [n_k][nq] int (device): the class
 *   with the largest sum of weights, the smallest such class on a tie.  The sums run in slot order from 0.
 * ava_kp_proba: the table is [nq][k]; out [nq][n_classes] float64 (device): the sums of weights of the classes
 *   0 .. n_classes - 1, in slot order, divided by the sum of all k weights (a sum of 0 counts as 1).
 *   1 <= n_classes <= ava_kp_max_classes() = 4096; a class code outside that range is counted in the divisor only.
 * ava_kp_regress: Y [n][n_out] float64 (device), 1 <= n_out <= ava_kp_max_outputs() = 256.  out [n_k][nq][n_out] float64
 *   (device): num / den with num = fma(w_s, Y[idx_s][t], num) and den += w_s over the slots in ascending order.
 * All return AVA_EINVAL before any launch for null pointers, an unknown dtype, a bad sweep or an unsupported shape. */
int ava_kp_max_sweep(void);
int ava_kp_max_classes(void);
int ava_kp_max_outputs(void);
int ava_kp_knn_masked(const void* x, int dtype, int n, int d, int k, const int* fold, int q0, int nq, int64_t* out_idx,
                      double* out_dist, ava_stream_t s);
int ava_kp_vote(const int64_t* idx, const double* dist, int nq, int kmax, const int* y, const int* ks, int n_k,
                int weighted, int* out_pred, ava_stream_t s);
int ava_kp_proba(const int64_t* idx, const double* dist, int nq, int k, const int* y, int n_classes, int weighted,
                 double* out, ava_stream_t s);
int ava_kp_regress(const int64_t* idx, const double* dist, int nq, int kmax, const double* Y, int n_out, const int* ks,
                   int n_k, int weighted, double* out, ava_stream_t s);

/* ---- Lloyd k-means with k-means++ seeding (row f25; csrc/kmeans.hip; scikit-learn 1.7 cluster/_kmeans.py:
 * _kmeans_plusplus, _tolerance, _kmeans_single_lloyd; _k_means_common.pyx: _relocate_empty_clusters_dense,
 * _inertia_dense) -----------------------------------------------------------------------------------------------------
 * x [n][d] (dtype 0 = float32, 1 = float64; device) is converted on load; everything else is fp64.  Every (row, centre)
 * and (row, row) distance has the bits ava_pair_sqdist gives the pair.  Nothing uses floating-point atomics: every sum
 * over rows is taken inside chunks of ava_km_chunk_rows() = 2048 rows in ascending row order and the chunk partials are
 * added in ascending chunk order, so the same inputs give the same bits on every run, for float32 and float64 copies of
 * the same values.  1 <= n <= 2^31 - 64, 1 <= d <= ava_km_max_d() = 128, 1 <= k <= ava_km_max_k() = 256; a fit also
 * needs k <= n.  Nothing allocates or synchronises; every pointer is a device pointer.
 * ws: ava_km_workspace_bytes(n, d, k) bytes (0 for an unsupported shape); ava_km_pp_step and ava_km_variance accept the
 *   size for k = 1.
 *
 * ava_km_assign: labels [n] int = the nearest of the centres [k][d] of every row, the lowest index on a tie; d2 [n] the
 *   squared distance to it; inertia [1] (may be null) = sum d2 in the chunk order.
 * ava_km_update: one M-step from labels [n] int (a label outside [0, k) is in no cluster): counts [k] int64 and
 *   centres [k][d] = the sum of the rows of the cluster in the chunk order / its count, zeros for an empty cluster.
 * ava_km_fit: iterations [it0, it0 + n_iters) of sklearn's Lloyd loop on centres [k][d] (in and out): assign, new centres
 *   (an empty cluster takes the row farthest from its own centre; several empty clusters in ascending id take the rows in
 *   the order (d2 descending, row ascending); the row leaves its old cluster's sum and count), shift = sum_k |c_new -
 *   c_old|^2; the loop stops when no label changed (strict), else when shift <= tol * mean_var[0].  labels [n] int must
 *   hold -1 before iteration 0; labels and d2 [n] are those of the last assignment that ran, made at the centres BEFORE
 *   that iteration's update.  ctl [>= 3 + it0 + n_iters] int, zeroed before iteration 0: ctl[0] = 1 after a strict stop,
 *   ctl[1] the number of iterations that ran, ctl[2 + it] whether the loop had stopped before iteration it: the launches
 *   of a stopped iteration return at once, so iterations are enqueued in blocks between reads of ctl.  shift [1] (may be
 *   null): the shift of the last iteration that ran.  mean_var [1]: ava_km_variance's out[0].
 * ava_km_pp_start: closest [n] = the squared distance of every row to row `first` (sklearn's first centre).
 * ava_km_pp_step: one further centre of sklearn's _kmeans_plusplus.  rand [n_trials] are the caller's uniform draws,
 *   1 <= n_trials <= 8.  The candidates are searchsorted(scan, rand * potential) clipped to n - 1, scan the inclusive
 *   sums of closest (sequential inside the chunks, the ascending chunk offsets added), potential its last entry; the
 *   candidate whose min(closest, d2(candidate, .)) has the least sum (chunk order; the first on a tie) is written to
 *   out_idx [1] int, its sum to out_pot [1], and closest becomes that minimum.
 * ava_km_variance: out [1 + d]: out[1 + j] = mean_n (x_nj - mean_j)^2 with both means in the chunk order, out[0] their
 *   ascending sum / d (np.mean(np.var(x, axis=0)), the factor of sklearn's _tolerance).
 * ava_km_transform: out [n][k] = the euclidean distance of every row to every centre (the square root of the tile).
 *
 * All return AVA_EINVAL before any launch for null pointers, an unknown dtype or an unsupported shape, AVA_EWORKSPACE
 * for a workspace that is too small. */
int ava_km_max_d(void);
int ava_km_max_k(void);
int ava_km_chunk_rows(void);
size_t ava_km_workspace_bytes(int n, int d, int k);
int ava_km_assign(const void* x, int dtype, int n, int d, int k, const double* centres, int* labels, double* d2,
                  double* inertia, void* ws, size_t ws_bytes, ava_stream_t s);
int ava_km_update(const void* x, int dtype, int n, int d, int k, const int* labels, double* centres, int64_t* counts,
                  void* ws, size_t ws_bytes, ava_stream_t s);
int ava_km_fit(const void* x, int dtype, int n, int d, int k, double* centres, int* labels, double* d2, double tol,
               const double* mean_var, int it0, int n_iters, int* ctl, double* shift, void* ws, size_t ws_bytes,
               ava_stream_t s);
int ava_km_pp_start(const void* x, int dtype, int n, int d, int first, double* closest, ava_stream_t s);
int ava_km_pp_step(const void* x, int dtype, int n, int d, int n_trials, const double* rand, double* closest, int* out_idx,
                   double* out_pot, void* ws, size_t ws_bytes, ava_stream_t s);
int ava_km_variance(const void* x, int dtype, int n, int d, double* out, void* ws, size_t ws_bytes, ava_stream_t s);
int ava_km_transform(const void* x, int dtype, int n, int d, int k, const double* centres, double* out, ava_stream_t s);

/* ---- Trustworthiness, continuity and preserved neighbours of an embedding (row f26; csrc/embed_quality.hip): the ava_eq_
 * entry points are declared, with their comment block, in a header of their own, mirrored by _lib.EQ_SIGNATURES -------- */
#include "ava_embed_quality.h"

/* ---- Connected components and the symmetric eigensolver of a sparse graph (row f27; csrc/spectral.hip): the ava_sp_
 * entry points are declared, with their comment block, in a header of their own, mirrored by _lib.SP_SIGNATURES -------- */
#include "ava_spectral.h"

#ifdef __cplusplus
}
#endif
#endif /* AVA_HIP_H */
