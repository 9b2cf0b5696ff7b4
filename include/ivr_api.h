/*
 * ivr_api.h - C ABI of libivr_hip.so: the MI355X (gfx950) implementation of the
 * frame -> embedding -> cosine top-k hot path of
 * DMDung2k3/Intelligent-Video-Analysis-Retrieval-System.
 *
 * The reference has no FFI of its own: the path sits behind duck-typed Python
 * objects.  Each entry point below names the reference call
 * it stands in for; paths are relative to the reference checkout.  The Python
 * mirror of the reference classes (ivr_amd/compat.py) binds these through ctypes
 * (ivr_amd/_ffi.py); INTEGRATION.md shows the stub a maintainer would add.
 *
 * Conventions
 *  - extern "C", plain pointers and sizes; no torch / numpy types.
 *  - Every bulk pointer marked DEV is a device (HBM) pointer owned by the caller;
 *    HOST pointers are small parameter blocks or one-time weight uploads.
 *  - `stream` is a hipStream_t passed as void* (NULL = the null stream).  Calls
 *    only enqueue work; nothing synchronises unless stated.
 *  - Every function returns IVR_OK (0) or a negative ivr_status and never throws
 *    or aborts; ivr_last_error() returns the calling thread's last message.
 *  - Handles may be used from several host threads (the reference calls
 *    encode_images from a 4-thread pool, unified_index.py:773): the host side of calls
 *    on one handle is serialised by a per-handle mutex, distinct handles are independent.
 *    A tower / index handle owns device workspaces (activations, search candidates), so
 *    all calls on ONE handle must be enqueued on ONE stream at a time: to move a handle
 *    to another stream, make the new stream wait for the old one first.  ivr_preprocess
 *    keeps its scratch per stream and may be called concurrently on different streams.
 */
#ifndef IVR_API_H
#define IVR_API_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define IVR_API_VERSION 11
#define IVR_MAX_K 2048          /* reference: k=50 default, SearchOptions.limit <= 1000 (system.py:91) */

typedef enum ivr_status {
    IVR_OK = 0,
    IVR_ERR_INVALID = -1,       /* bad argument / shape: shim raises ValueError (core.py:1178-1191) */
    IVR_ERR_HIP = -2,           /* HIP runtime failure: shim raises RuntimeError (core.py:894-896) */
    IVR_ERR_OOM = -3,
    IVR_ERR_STATE = -4,         /* handle not ready (e.g. tower not finalized, index empty where rows are needed) */
    IVR_ERR_UNSUPPORTED = -5
} ivr_status;

typedef struct ivr_ctx ivr_ctx;
typedef struct ivr_index ivr_index;
typedef struct ivr_tower ivr_tower;
typedef void *ivr_stream;

/* ---- context ------------------------------------------------------------------------------- */
int ivr_api_version(void);
int ivr_init(int device, ivr_ctx **out);
int ivr_destroy(ivr_ctx *ctx);
const char *ivr_last_error(ivr_ctx *ctx);       /* ctx may be NULL */
int ivr_device_info(ivr_ctx *ctx, int *cu_count, int64_t *hbm_bytes, char *arch, int arch_len);
/* Device scratch (ivr_preprocess intermediates, ivr_frame_quality planes, ...) is kept per stream and only grows.  A caller that
 * retires a stream (and every graph captured on it) hands its block back with this call: it waits for the stream, frees the block
 * and forgets the stream, so a recycled stream handle starts clean.  No-op for a stream that never used scratch. */
int ivr_release_stream_scratch(ivr_ctx *ctx, ivr_stream stream);

/* ---- measurement hooks (bench.py): per-kernel HIP-event timing on the launch stream ---------------
 * No counterpart in the reference (its only profiler is the wall-clock PerformanceMonitor.timer,
 * utils.py:2481).  on = 1 brackets every launch of the kernels that carry a step (GEMMs, LayerNorm,
 * attention, index scans, preprocess emit) with two events; on = 2 also the short launches of the search
 * tail and the index append (an event pair costs microseconds on the stream: too much to leave around
 * 5-microsecond kernels inside a timed region).  ivr_profile_json synchronises on the events and writes
 * {"kernel": {"launches", "ms", "work"}} where work is the launch's algorithmic bytes (HBM-bound kernels)
 * or FLOP (MFMA-bound kernels). */
int ivr_profile_enable(ivr_ctx *ctx, int on);
int ivr_profile_reset(ivr_ctx *ctx);
int ivr_profile_json(ivr_ctx *ctx, char *buf /*HOST*/, int len);

/* ---- P1 / P2: frame preprocessing -------------------------------------------------------------
 * Replaces HFCLIPProcessor(images=...) at core.py:1613 and
 * cv2.cvtColor + Image.resize + processor(...) at video_frame_filter.py:58-59,29.
 * src: DEV uint8 [n, h, w, 3] (NHWC, dense).  Output: [n,3,S,S] (NCHW) or the patch-major
 * im2col matrix [n*(S/P)^2, 3*P*P] (column order c,py,px = the conv weight's) that feeds the
 * patch-embed GEMM directly.  Geometry is PIL's two-pass fixed-point resampler, bit-exact.
 */
enum {
    IVR_PP_MODE_IDENTITY = 0,           /* h == w == S */
    IVR_PP_MODE_SHORTEST_EDGE_CROP = 1, /* CLIP processor: shortest edge -> S, centre crop SxS */
    IVR_PP_MODE_STRETCH = 2,            /* video_frame_filter.py:59 */
    IVR_PP_MODE_LETTERBOX = 3,          /* extra (BASELINE.json wording); long edge -> S, zero canvas */
    IVR_PP_MODE_MASK = 0xF,
    IVR_PP_BGR = 1 << 4,                /* src is BGR (cv2) - swapped while loading */
    IVR_PP_OUT_F32 = 1 << 5,            /* default output dtype is bf16 */
    IVR_PP_OUT_PATCH_MAJOR = 1 << 6,    /* default layout is NCHW */
    IVR_PP_BILINEAR = 1 << 7            /* default filter is BICUBIC (PIL default, CLIP processor) */
};
int ivr_preprocess(ivr_ctx *ctx, const uint8_t *src /*DEV*/, int n, int h, int w, int flags,
                   const float mean[3] /*HOST*/, const float std[3] /*HOST*/, int out_size, int patch,
                   void *dst /*DEV*/, ivr_stream stream);
/* bytes of DEV scratch ivr_preprocess needs for (n,h,w,flags); 0 for identity geometry.  The scratch
 * lives in the context, one block per stream, and grows on demand (outside of stream capture); outgrown
 * blocks stay allocated until ivr_destroy because kernels in flight or a captured graph may still use them. */
int64_t ivr_preprocess_scratch_bytes(int n, int h, int w, int flags, int out_size);

/* The geometry stage of ivr_preprocess on its own: src DEV uint8 [n,h,w,3] -> dst DEV uint8 [n,S,S,3], S = out_size, the same
 * Pillow-exact resampler (flags: one IVR_PP_MODE_* and IVR_PP_BILINEAR; every other bit is rejected).  The channel order is left as
 * it came.  Replaces Image.fromarray(img_rgb).resize(FRAME_SIZE) at filter_research_update.py:246, whose result the reference both
 * embeds and hashes.  Scratch: ivr_preprocess_scratch_bytes. */
int ivr_resize_u8(ivr_ctx *ctx, const uint8_t *src /*DEV*/, int n, int h, int w, int flags, int out_size, uint8_t *dst /*DEV*/,
                  ivr_stream stream);

/* ---- perceptual hash ---------------------------------------------------------------------------------
 * Replaces imagehash.phash(img) at filter_research_update.py:97-99 (called per frame at :250) for a batch of frames already in HBM.
 * src: DEV uint8 [n,h,w,3], 1 <= h, w <= IVR_PHASH_MAX_SIDE; flags: 0 or IVR_PP_BGR.  Per frame:
 *   grey    (R*19595 + G*38470 + B*7471 + 0x8000) >> 16                                   (Pillow convert('L'))
 *   resize  to 32x32, Pillow's 8-bit resampler with the Lanczos filter (support 3): horizontal pass first, uint8 between the
 *           passes, a pass skipped when that axis is already 32.  pixels (DEV uint8 [n,32,32], or NULL) receives this image
 *   DCT     float64, type II, unnormalised, columns then rows, the low 8x8 block: with C[k][m] = cos(pi k (2m+1) / 64)
 *           (ivr_phash_cos_table), A[k][x] = 2 sum_y C[k][y] p[y][x] and B[k][l] = 2 sum_x A[k][x] C[l][x], both sums in ascending
 *           order, every product and sum rounded on its own (no fma)
 *   bits    B[k][l] > (s[31] + s[32]) / 2 over the sorted 64 values s; packed row-major, most significant bit first
 * hash: DEV uint8 [n,8]; its hex form is str(imagehash.phash(img)).  Two launches (grey + horizontal pass over bands of rows, then one
 * workgroup per frame); the scratch between them ([n,h,32] bytes) lives in the context, per stream. */
#define IVR_PHASH_MAX_SIDE 8192
int64_t ivr_phash_scratch_bytes(int n, int h, int w);
int ivr_phash(ivr_ctx *ctx, const uint8_t *src /*DEV*/, int n, int h, int w, int flags, uint8_t *hash /*DEV*/,
              uint8_t *pixels /*DEV or NULL*/, ivr_stream stream);
/* out[k * 32 + m] = C[k][m] for k < 8, m < 32: the 256 doubles the kernel multiplies with (computed on the host; needs no GPU) */
int ivr_phash_cos_table(double *out /*HOST [256]*/);

/* ---- E1 / E2 / E3 + N1: encoder towers --------------------------------------------------------
 * Replaces CLIPModel.get_image_features + F.normalize (core.py:1619-1620),
 * CLIPModel.get_text_features + F.normalize (core.py:1541-1542) and
 * ViTModel(...).last_hidden_state[:,0,:] (video_frame_filter.py:31-32).
 */
enum { IVR_ACT_QUICK_GELU = 0, IVR_ACT_GELU_ERF = 1 };
enum { IVR_POOL_CLS_POSTLN_PROJ = 0, IVR_POOL_LN_ALL_CLS = 1, IVR_POOL_EOS_LN_PROJ = 2 };
enum { IVR_KIND_VISION = 0, IVR_KIND_TEXT = 1 };
enum {
    IVR_COMPUTE_BF16 = 0,
    IVR_COMPUTE_F32 = 1, /* verification mode: f32 MFMA, f32 activations */
    IVR_COMPUTE_FP8 = 2  /* BASELINE config 5: the linear sites of every block named by desc.fp8_sites on the CDNA4 fp8 MFMA
                          * (e4m3 operands, per-output-channel weight scales, f32 accumulate), the other sites on the bf16 MFMA;
                          * patch embedding, attention products, LN, residual stream and projection as in the bf16 mode */
};
/* the four linear sites of a transformer block (modeling_clip.py:259-277 q/k/v/out_proj, :338-350 fc1/fc2) */
enum { IVR_FP8_SITE_QKV = 1, IVR_FP8_SITE_ATTN_OUT = 2, IVR_FP8_SITE_FC1 = 4, IVR_FP8_SITE_FC2 = 8, IVR_FP8_SITE_ALL = 15 };

typedef struct ivr_tower_desc {
    int kind, width, layers, heads, mlp, tokens, out_dim, act, pool;
    int image, patch, pre_ln, patch_bias;   /* vision */
    int vocab, eos_id, causal;               /* text */
    int compute;                             /* IVR_COMPUTE_* */
    float ln_eps;
    /* IVR_COMPUTE_FP8 only.  fp8_sites: mask of IVR_FP8_SITE_* that run in e4m3 (0 = all four).  fp8_mlp_cls_bf16 = 1:
     * the rows of token 0 (CLS, the only row the vision pooling reads) go through fc1 / fc2 in bf16 on a side path
     * (n rows per launch instead of n*tokens), the e4m3 GEMMs leave those residual rows alone.  Which assignment stays
     * inside which tolerance: DESIGN.md section 4, profiles/r02_fp8_error_budget.json. */
    int fp8_sites, fp8_mlp_cls_bf16;
    /* IVR_COMPUTE_FP8 only: the mask applies to blocks fp8_first_layer .. layers-1, earlier blocks run in bf16 (the early
     * blocks are the sensitive ones: their error passes through every later attention).  0 = every block. */
    int fp8_first_layer;
} ivr_tower_desc;

int ivr_tower_create(ivr_ctx *ctx, const ivr_tower_desc *desc, ivr_tower **out);
/* name = canonical tensor name (ivr_amd/weights.py); data = HOST float32, nn.Linear layout W[out,in]. */
int ivr_tower_set_weight(ivr_tower *t, const char *name, const float *data /*HOST*/, int64_t count);
/* checks that every tensor was set, packs QKV, allocates the activation workspace for max_batch. */
int ivr_tower_finalize(ivr_tower *t, int max_batch);
int ivr_tower_destroy(ivr_tower *t);
/* patches: DEV patch-major pixels from ivr_preprocess (bf16, or f32 for IVR_COMPUTE_F32),
 * out: DEV float32 [n, embed_dim]; normalize=1 applies x / max(||x||, 1e-12) (F.normalize). */
int ivr_tower_encode_image(ivr_tower *t, const void *patches /*DEV*/, int n, int normalize,
                           float *out /*DEV*/, ivr_stream stream);
/* ids: DEV int64 [q, T] (T <= desc.tokens); pooled at the first eos_id per row. */
int ivr_tower_encode_text(ivr_tower *t, const int64_t *ids /*DEV*/, int q, int T, int normalize,
                          float *out /*DEV*/, ivr_stream stream);
/* bring-up / parity: arm a one-shot capture - the NEXT encode call copies the residual stream after
 * `layer` blocks (0 = embeddings) into out as f32 [n,T,width]. */
int ivr_tower_debug_hidden(ivr_tower *t, int layer, int n, float *out /*DEV*/, ivr_stream stream);
/* bring-up / parity: stage capture.  Each call arms one more copy for the NEXT encode call of this tower: straight after the launch
 * that produced the buffer of (layer, site), the encode call copies it to dst on its own stream (the workspace buffers are reused
 * from stage to stage, so the copy sits at that point of the stream), raw, in the buffer's own dtype (float32, bf16 or e4m3; eos_pos
 * int32).  The armed set clears when that call returns.  Unlike ivr_tower_debug_hidden at layer == layers, an armed capture never
 * changes the path the call takes: a pruned last block stays pruned.  With nothing armed the encode path pays one test per stage.
 * Extent copied (n = the call's batch, T its tokens, B = max_batch): the full-size buffers their n*T rows; the compact buffers
 * (LN2 of a pruned block, LN2_CLS, HID_CLS, HID_CLS8, EOS_POS, POOL_LN, POOLED) all B rows, so that the rows behind the n written
 * ones can be seen to keep their bits.  dst_bytes below that extent fails the encode call with IVR_ERR_INVALID.
 * layer: block index in [0, layers) for the per-block sites; [0, layers] for STREAM; 0 for EMBED, EOS_POS, POOL_LN, POOLED. */
enum {
    IVR_SITE_EMBED = 0,     /* f32 [n*T, width]: the residual stream after the embedding kernels, before the pre-LN */
    IVR_SITE_EOS_POS = 1,   /* int32 [B] (text towers) */
    IVR_SITE_STREAM = 2,    /* f32 [n*T, width]: the residual stream after `layer` blocks, as ivr_tower_debug_hidden gives it */
    IVR_SITE_LN1 = 3,       /* [n*T, width]: LN1 output, in the dtype of the QKV site's operand */
    IVR_SITE_QKV = 4,       /* [n*T, 3 width]; not materialised by the fused QKV + attention kernel */
    IVR_SITE_ATT = 5,       /* [n*T, width]: attention output, dtype of the attn-out operand (pruned + fused: compact rows [0, n)) */
    IVR_SITE_ATTN_OUT = 6,  /* f32 [n*T, width]: the residual stream after attn-out */
    IVR_SITE_LN2 = 7,       /* LN2 output, dtype of the fc1 operand: [n*T, width], or the token-0 rows [B, width] in a pruned block */
    IVR_SITE_LN2_CLS = 8,   /* bf16 [B, width]: LN2 of the token-0 rows for the fp8 side path */
    IVR_SITE_HID = 9,       /* [n*T, mlp]: fc1 output (e4m3 where fc1 and fc2 both are) */
    IVR_SITE_HID8 = 10,     /* e4m3 [n*T, mlp]: converted copy of a bf16 HID for an e4m3 fc2, behind B * tokens bf16 rows */
    IVR_SITE_HID_CLS = 11,  /* [B, mlp]: fc1 output of the token-0 rows (side path, pruned block) */
    IVR_SITE_HID_CLS8 = 12, /* e4m3 [B, mlp]: its converted copy, behind B bf16 rows */
    IVR_SITE_FC2 = 13,      /* f32 [n*T, width]: the residual stream after the full-size fc2, before the side path adds its rows */
    IVR_SITE_POOL_LN = 14,  /* [B, width]: the pooled rows after the final LN (bf16 / f32; f32 for IVR_POOL_LN_ALL_CLS) */
    IVR_SITE_POOLED = 15,   /* f32 [B, embed_dim]: the embedding before F.normalize */
    IVR_SITE_COUNT = 16
};
int ivr_tower_debug_capture(ivr_tower *t, int layer, int site, void *dst /*DEV*/, int64_t dst_bytes);
/* capture `index` (arming order) of the last encode call that had captures armed: bytes copied (0: the path the call took does not
 * materialise that site) and the bytes per element of the buffer's dtype. */
int ivr_tower_debug_capture_result(ivr_tower *t, int index, int64_t *bytes /*HOST*/, int *elem_bytes /*HOST*/);
int64_t ivr_tower_workspace_bytes(ivr_tower *t);

/* Building block of the towers, exposed for parity tests and kernel benchmarks: y = x W^T (+ bias), i.e. the
 * nn.Linear calls inside the HF modules (modeling_clip.py:259-277, 338-350).  x: DEV [M,K], w: DEV [N,K], both
 * bf16 (f32_mode = 0) or float32 (f32_mode = 1); bias: DEV float32 [N] or NULL.  K must be a multiple of 64 (32 in f32 mode),
 * N of 4.  epilogue 0: out = act(y) in the operand dtype (act = -1 none, else IVR_ACT_*); 1: resid (DEV float32 [M,N]) += y;
 * 3: out = y as float32. */
int ivr_linear(ivr_ctx *ctx, int f32_mode, int epilogue, const void *x /*DEV*/, const void *w /*DEV*/,
               const float *bias /*DEV*/, int M, int N, int K, int act, void *out /*DEV*/, float *resid /*DEV*/,
               ivr_stream stream);

/* fp8 variant of ivr_linear (the GEMM of IVR_COMPUTE_FP8): x DEV [M,K] and w DEV [N,K] are OCP e4m3 bytes, colscale DEV
 * float32 [N] multiplies column n of x w^T before the bias (the weight's dequantisation scale; NULL = 1).  K % 128 == 0,
 * N % 64 == 0.  epilogue 0: out = act(y) as bf16 (out_fp8 = 0) or saturated e4m3 (out_fp8 = 1); 1: resid += y. */
int ivr_linear_fp8(ivr_ctx *ctx, int epilogue, const void *x /*DEV*/, const void *w /*DEV*/, const float *colscale /*DEV*/,
                   const float *bias /*DEV*/, int M, int N, int K, int act, void *out /*DEV*/, int out_fp8,
                   float *resid /*DEV*/, ivr_stream stream);

/* Every GEMM call site of the towers, exposed for the per-element tests: the GemmArgs fields the towers set, routed through the
 * same launchers (kernel choice, slabs of row operands beyond 2 GiB and the IVR_GEMM* switches included).
 *   y[m, n] = sum_k A[m*lda + k] W[n*ldw + k] (* colscale[n], e4m3 only) (+ bias[n])
 *   IVR_EPI_STORE: out[m*ldo + n] = act(y) in the operand dtype (e4m3: bf16, or saturated e4m3 bytes with out8 = 1)
 *   IVR_EPI_RESID: resid[m*ldr + n] += y, except rows m % skip_mod == 0 (skip_mod > 0), which are left untouched
 *   IVR_EPI_PATCH: resid[((m / G2) * T + 1 + m % G2) * ldr + n] = y + pos[(1 + m % G2) * N + n] (patch embedding: token 0 of every
 *                  image is not written); bf16 / float32 operands, M % G2 == 0, T > G2
 *   IVR_EPI_F32:   out[m*ldo + n] = y as float32 (bf16 / float32 operands)
 * Limits: bf16 K % 64 == 0, float32 K % 32 == 0, N % 4 == 0; e4m3 K % 128 == 0, N % 64 == 0, lda and ldw % 16 == 0.  K <= lda, ldw;
 * N <= ldo (STORE, F32), ldr (RESID, PATCH); every leading dimension at most 2^21, lda and ldw whole multiples of 16 bytes, ldo and
 * ldr multiples of 4 (e4m3 output: ldo % 16 == 0, bf16 output of e4m3: ldo % 8 == 0), pointers 16-byte aligned.  act (IVR_ACT_*, -1 none) only with IVR_EPI_STORE, skip_mod only with IVR_EPI_RESID, colscale and out8 only with e4m3.
 * reverse_m = 1 walks the row panels from the last to the first (same result).  M = 0 is a no-op. */
enum { IVR_GEMM_BF16 = 0, IVR_GEMM_F32 = 1, IVR_GEMM_E4M3 = 2 };
enum { IVR_EPI_STORE = 0, IVR_EPI_RESID = 1, IVR_EPI_PATCH = 2, IVR_EPI_F32 = 3 };
typedef struct ivr_gemm_desc {
    int dtype, epilogue, act;            /* IVR_GEMM_*, IVR_EPI_*, -1 or IVR_ACT_* */
    int M, N, K;
    const void *A;                       /* DEV [M, lda] */
    int lda;
    const void *W;                       /* DEV [N, ldw] */
    int ldw;
    const float *bias, *colscale;        /* DEV float32 [N] or NULL */
    void *out;                           /* DEV [M, ldo] */
    int ldo, out8;
    float *resid;                        /* DEV float32: [M, ldr] (RESID), [(M / G2) * T, ldr] (PATCH) */
    int ldr;
    const float *pos;                    /* DEV float32 [T, N] (PATCH) */
    int T, G2, skip_mod, reverse_m;
} ivr_gemm_desc;
int ivr_gemm(ivr_ctx *ctx, const ivr_gemm_desc *desc, ivr_stream stream);

/* Attention of the towers, exposed for parity tests and kernel benchmarks: att[n*T, D] = softmax(Q K^T [+ causal mask]) V per
 * (image, head), the scaled_dot_product_attention inside the HF attention modules (modeling_clip.py:259-277).  qkv: DEV
 * [n*T, 3D], row = q | k | v, head h at columns h*64 .. h*64+63 of each part; no 1/sqrt(64) scale is applied (the towers fold it
 * into the Q weights).  f32_mode = 1: qkv / att float32, T <= 301 (K and V of a head in LDS), n <= 65535; else qkv bf16 and att
 * bf16 (out_fp8 = 0) or saturated OCP e4m3 (out_fp8 = 1, only where a kernel writes it: T <= 640).  D = 64 * heads, 1 <= heads <= 32,
 * 1 <= T <= 1024, pointers 16-byte aligned; n = 0 is a no-op (qkv / att may be NULL). */
int ivr_attention(ivr_ctx *ctx, int f32_mode, const void *qkv /*DEV*/, int n, int T, int D, int heads, int causal, int out_fp8,
                  void *att /*DEV*/, ivr_stream stream);
/* Fused variant: qkv = xn W^T + bias rounded to bf16, then ivr_attention (not causal); xn DEV bf16 [n*T, D], w DEV bf16 [3D, D],
 * bias DEV float32 [3D].  T <= 64, D = 64 * heads >= 192, n * T * D * 2 < 2^31, pointers 16-byte aligned; n = 0 is a no-op. */
int ivr_qkv_attention(ivr_ctx *ctx, const void *xn /*DEV*/, const void *w /*DEV*/, const float *bias /*DEV*/, int n, int T, int D,
                      int heads, int out_fp8, void *att /*DEV*/, ivr_stream stream);
/* LayerNorm of the towers (nn.LayerNorm, modeling_clip.py:332-336): out row r = LN(x row r*row_mul + (offs ? offs[r] : 0)) with
 * g, b DEV float32 [D]; x DEV float32; offs DEV int32 [rows] or NULL; out_kind 0 bf16, 1 float32, 2 saturated e4m3;
 * reverse = 1 walks the rows backwards (same result).  D % 4 == 0, D <= 2048, pointers 16-byte aligned; rows = 0 is a no-op. */
int ivr_layernorm(ivr_ctx *ctx, int out_kind, const float *x /*DEV*/, int row_mul, const int *offs /*DEV*/, const float *g /*DEV*/,
                  const float *b /*DEV*/, float eps, int rows, int D, int reverse, void *out /*DEV*/, ivr_stream stream);

/* The weight quantiser of IVR_COMPUTE_FP8, exposed so that it can be checked without a GPU: HOST float32 -> HOST OCP e4m3 bytes
 * (bias 7, no infinity, max 448), round to nearest even, saturating; NaN -> 0x7f | sign. */
int ivr_quantize_e4m3_host(const float *src /*HOST*/, uint8_t *dst /*HOST*/, int64_t n);

/* ---- N2 / N3: row L2 normalisation -------------------------------------------------------------
 * Replaces FAISSRetriever._normalize_and_validate_features (core.py:1176-1196) and
 * faiss.normalize_L2 (unified_index.py:1776): x /= ||x||, all-zero rows stay zero.  In place.
 * nonfinite (DEV int32, may be NULL) receives the count of NaN/Inf input elements (the shim turns
 * a non-zero count into the ValueError of core.py:1190-1191).
 */
int ivr_l2_normalize(ivr_ctx *ctx, float *x /*DEV*/, int64_t n, int d, int32_t *nonfinite /*DEV*/,
                     ivr_stream stream);

/* ---- I1 + S1: flat inner-product index ---------------------------------------------------------
 * Replaces faiss.IndexFlatIP(d) / .add / .search (unified_index.py:1767,1779,503; core.py:1208,827,891).
 * Rows live in HBM as float32 in a 16-row x 4-float interleaved tile layout chosen so that one
 * wave-wide 16-byte load is an MFMA operand fragment and 1 KiB contiguous.
 */
int ivr_index_create(ivr_ctx *ctx, int d, int64_t capacity_rows, ivr_index **out);
int ivr_index_destroy(ivr_index *idx);
int ivr_index_reset(ivr_index *idx);                        /* ntotal = 0; plain or id-mapped is undecided again */
int64_t ivr_index_ntotal(ivr_index *idx);
int ivr_index_dim(ivr_index *idx);
int64_t ivr_index_capacity(ivr_index *idx);
/* append n rows (DEV float32 [n,d] row-major); grows the allocation when capacity is exceeded. */
int ivr_index_add(ivr_index *idx, const float *rows /*DEV*/, int64_t n, int normalize, ivr_stream stream);
/* overwrite rows [start, start+n) (ring-buffer use, BASELINE config 4); start+n <= ntotal. */
int ivr_index_write(ivr_index *idx, int64_t start, const float *rows /*DEV*/, int64_t n, int normalize,
                    ivr_stream stream);
/* rolling-window variant for a captured (hipGraph) streaming step: overwrite the n rows at *cursor (DEV int64, a multiple of
 * n; n must divide ntotal) and advance the cursor by n modulo ntotal, all on the stream. */
int ivr_index_write_ring(ivr_index *idx, const float *rows /*DEV*/, int64_t n, int normalize, int64_t *cursor /*DEV*/,
                         ivr_stream stream);
/* copy rows [start, start+n) back to row-major float32 (faiss reconstruct_n). */
int ivr_index_reconstruct(ivr_index *idx, int64_t start, int64_t n, float *out /*DEV*/, ivr_stream stream);
/* pre-size the search workspace so that ivr_index_search allocates nothing (hipGraph capture). */
int ivr_index_reserve_search(ivr_index *idx, int max_nq, int max_k);
/* Exact top-k by inner product.  q: DEV float32 [nq,d]; D: DEV float32 [nq,k] descending;
 * I: DEV int64 [nq,k] = id_base + row, ties broken by lower id; unused slots (-FLT_MAX, -1). */
int ivr_index_search(ivr_index *idx, const float *q /*DEV*/, int nq, int k, int normalize_q,
                     int64_t id_base, float *D /*DEV*/, int64_t *I /*DEV*/, ivr_stream stream);
/* Diagnostics of the bf16 candidate scan behind ivr_index_search: HOST out[0] = 1 when the index keeps a bf16
 * scan copy, out[1] = number of queries of the LAST scan chunk (<= 64 queries) whose verification failed and which were redone by
 * the exact float32 scan.  Synchronises the device. */
int ivr_index_scan_stats(ivr_index *index, int *out /*HOST [2]*/);
/* Exact range search by inner product: for each query, every stored row with <q, row> > radius (strict, as faiss does for
 * METRIC_INNER_PRODUCT).  lims: DEV int64 [nq+1], lims[0] = 0, results of query i at [lims[i], lims[i+1]), ids ascending
 * within a query (id = id_base + row).  D/I: DEV, capacity `cap` entries; entries at positions >= cap are counted in lims
 * but not written (the caller re-calls with cap >= lims[nq]).  Enqueues only: no host synchronisation.
 * Scores are bit-identical to the ones ivr_index_search reports for the same rows.  radius must not be NaN (+-inf are allowed);
 * an empty index gives all-zero lims. */
int ivr_index_range_search(ivr_index *idx, const float *q /*DEV*/, int nq, float radius, int normalize_q, int64_t id_base,
                           int64_t *lims /*DEV*/, float *D /*DEV*/, int64_t *I /*DEV*/, int64_t cap, ivr_stream stream);

/* Filtered search (faiss SearchParameters(sel=IDSelector...)): which ids a filtered search may return (id = id_base + row).  An id is
 * allowed iff lo <= id < hi and, when bits != NULL, id < nbits && ((bits[id >> 3] >> (id & 7)) & 1): faiss IDSelectorBitmap order =
 * numpy.packbits(mask, bitorder="little").  A bitmap byte is only read for an id inside [lo, hi), so bits may point in front of the
 * caller's buffer by the bytes below lo >> 3. */
typedef struct ivr_id_filter {
    int64_t lo, hi;          /* lo >= hi: nothing allowed */
    const uint8_t *bits;     /* DEV, or NULL: the range alone */
    int64_t nbits;           /* >= 0 */
} ivr_id_filter;
/* ivr_index_search / ivr_index_range_search limited to the allowed rows: top k (or every row above radius) among them only, ties to the
 * lower id, unused slots (-FLT_MAX, -1); each score is bit-identical to the one ivr_index_search reports for that row.  Only the 64-row
 * groups that overlap the allowed id range are scanned.  Enqueues only (no host synchronisation) and allocates nothing the unfiltered
 * call would not.  filter: HOST, read during the call; NULL = the unfiltered call. */
int ivr_index_search_filtered(ivr_index *idx, const float *q /*DEV*/, int nq, int k, int normalize_q, int64_t id_base,
                              const ivr_id_filter *filter /*HOST*/, float *D /*DEV*/, int64_t *I /*DEV*/, ivr_stream stream);
int ivr_index_range_search_filtered(ivr_index *idx, const float *q /*DEV*/, int nq, float radius, int normalize_q, int64_t id_base,
                                    const ivr_id_filter *filter /*HOST*/, int64_t *lims /*DEV*/, float *D /*DEV*/, int64_t *I /*DEV*/,
                                    int64_t cap, ivr_stream stream);

/* faiss IndexFlat::remove_ids(sel): delete every stored row whose id (id_base + row) the filter allows.  The filter is read exactly as
 * ivr_index_search_filtered reads it (lo <= id < hi, the optional bitmap in faiss order, ids outside [id_base, id_base + ntotal) match
 * nothing), but it is required: filter == NULL and nbits < 0 are IVR_ERR_INVALID, there is no "remove everything" default; a filter
 * that matches no stored row is a no-op that returns IVR_OK with *n_removed = 0.
 * The surviving rows keep their relative order and move down to rows 0 .. ntotal' - 1 (as in faiss, the ids above a removed row
 * shift); ntotal becomes ntotal', *n_removed (HOST, may be NULL) receives ntotal - ntotal', the capacity does not change.  Every
 * surviving row keeps its bits in the float32 tiles and in the bf16 scan copy, so a search after the call reports for a surviving row
 * the bit-identical score it reported before.  Rows [ntotal', old ntotal) are zero in both layouts afterwards, down to the slots of
 * a partly filled 16-row tile: the state ivr_index_create and ivr_index_reset establish.  The bounds of the bf16 candidate scan
 * (largest row norm, largest |row - bf16(row)|) are upper bounds over the rows ever stored; they stay valid and are left alone.
 * Cost follows the tail: rows below the first removed row are neither read nor written, and the filter is evaluated from the
 * 256-row block of its first allowed row on.  The extra device memory is a bounce buffer of at most IVR_REMOVE_CHUNK_ROWS rows in
 * both layouts (environment, read by ivr_index_create; default 65536) plus 12 bytes per 64 rows of the tail.
 * Synchronises `stream` once (the host needs the count to set ntotal): the call cannot be captured into a hipGraph, and a graph
 * captured on this index before the call holds the old ntotal.  One stream at a time per handle, as for every call. */
int ivr_index_remove_ids(ivr_index *idx, int64_t id_base, const ivr_id_filter *filter /*HOST*/, int64_t *n_removed /*HOST, may be NULL*/,
                         ivr_stream stream);

/* ---- stable external ids (faiss IndexIDMap2 / add_with_ids) --------------------------------------
 * The reference keys its metadata by FAISS id (core.py:722-723: id_to_metadata / metadata_to_id) and looks rows up by it
 * (search_by_id, core.py:932-958).  With row positions as ids every key above a removed row goes stale; an id-mapped index
 * carries caller-chosen int64 labels with its rows instead: a device table ids[capacity], ids[r] = the label of stored row r.
 *
 * An index becomes id-mapped by ivr_index_add_with_ids while it is empty and stays so until ivr_index_reset; a plain index (the
 * one ivr_index_add makes) is not touched by any of this.  ivr_index_add_with_ids on a non-empty plain index and ivr_index_add
 * on an id-mapped index (faiss IndexIDMap::add throws too) return IVR_ERR_STATE; n == 0 on an empty index only decides the mode.
 * ids: DEV int64 [n], every id >= 0 (-1 labels an unused result slot and the filters never match a negative id; the caller
 * checks, the ids are not read on the host).  Duplicate ids are allowed, as in faiss: every row is treated on its own.  The
 * table grows with the rows and keeps its contents; ivr_index_write and ivr_index_write_ring replace vectors and leave ids alone.
 *
 * On an id-mapped index every entry point above keeps its signature, and
 *  - id_base is ignored;
 *  - labels written to I are ids[row], unused slots stay -1; order and ties follow the storage order as before (equal scores:
 *    the lower row first whatever its label; range-search results of a query in ascending row order);
 *  - a filter names stored ids.  One pass over the table (8 bytes read per stored row, one bit written) turns it into a row
 *    bitmap, then the masked kernels run over the WHOLE index: unlike on a plain index a narrow id range does not narrow the
 *    scan.  A byte of filter->bits is read only for a stored id inside [max(lo, 0), min(hi, nbits)).  Still enqueue-only: no
 *    host synchronisation, and after ivr_index_reserve_search no allocation until the index grows;
 *  - ivr_index_remove_ids compacts the table with the rows; ids at or above the new ntotal are never read. */
int ivr_index_add_with_ids(ivr_index *idx, const float *rows /*DEV*/, const int64_t *ids /*DEV*/, int64_t n, int normalize,
                           ivr_stream stream);
int ivr_index_has_ids(ivr_index *idx);                      /* 1: id-mapped, 0: plain (or NULL) */
/* ids[start .. start + n) -> out (faiss id_map[start:start+n]); start + n <= ntotal; IVR_ERR_STATE on a plain index. */
int ivr_index_get_ids(ivr_index *idx, int64_t start, int64_t n, int64_t *out /*DEV*/, ivr_stream stream);
/* rows[i] = the lowest row that holds id keys[i], or -1 (what IndexIDMap2::reconstruct and the reference's search_by_id,
 * core.py:932-958, need); a negative key and any key on an empty index give -1.  Two paths with the same results:
 *  - n < IVR_FIND_TABLE_MIN_KEYS: one scan of the whole id table per call, O(n x ntotal) compares, nothing allocated;
 *  - otherwise a device hash table from stored id to lowest row: open addressing with linear probing, a power-of-two number of
 *    slots >= 2 ntotal (load factor <= 1/2, 16 bytes per slot: at most 64 bytes per stored row), the id bits mixed before masking,
 *    empty key -1.  Nothing is allocated until the first lookup that takes this path.  The table is built by one pass over
 *    ids[0 .. ntotal) (a 64-bit compare-and-swap claims a key's slot, an atomic minimum lowers its row, so duplicates resolve to
 *    the lowest row as the scan does); ivr_index_add_with_ids, ivr_index_remove_ids and ivr_index_reset mark it stale, the next
 *    lookup rebuilds it, ivr_index_reset and ivr_index_destroy free it.
 * A lookup that builds or rebuilds the table allocates and so cannot be captured into a hipGraph; one that finds the table built,
 * and the scan path, only enqueue.  IVR_FIND_TABLE_MIN_KEYS (environment, read by ivr_index_create; 0 = always the table, a huge
 * value = always the scan) defaults to 512: the smallest measured key count at which a table lookup including one
 * rebuild beats the scan on 1M rows (0.161 ms against 0.171 ms; a built table answers any number of keys up to 65,536 in 0.025 ms). */
int ivr_index_find_ids(ivr_index *idx, const int64_t *keys /*DEV*/, int64_t n, int64_t *rows /*DEV*/, ivr_stream stream);

/* ---- row access by position: gather, scatter, search + reconstruct ---------------------------------
 * Random access to the stored rows over both layouts (the float32 tiles and the bf16 scan copy).  One row of d floats is d / 4
 * pieces of 16 bytes spaced 256 bytes apart inside its 16-row tile, so a random row touches every cache line of its tile: 16 times
 * the row's bytes move on the index side ("row access").  The row-major side of both calls is fully coalesced.
 * Both are positional on plain and id-mapped indexes alike (ivr_index_find_ids turns stored ids into rows), enqueue-only, and
 * n == 0 is a no-op.
 *
 * ivr_index_gather: faiss reconstruct_batch(n, keys, out).  out[i] = stored row rows[i] as row-major float32 with the exact bits
 * ivr_index_reconstruct returns; an entry outside [0, ntotal) (-1, the empty result slot, included) gives a row of d NaNs, what
 * faiss::Index::search_and_reconstruct writes for a -1 label.  Repeats are allowed.  rows: DEV int64 [n], out: DEV [n,d]. */
int ivr_index_gather(ivr_index *idx, const int64_t *rows /*DEV*/, int64_t n, float *out /*DEV*/, ivr_stream stream);
/* ivr_index_scatter: faiss IndexIVF::update_vectors applied to the flat index, and the n calls ivr_index_write(rows[i], x + i d, 1,
 * normalize) of unified_index.py's modified-file loop in one launch.  Stored row rows[i] becomes x[i] in the float32 tiles and in
 * the bf16 scan copy, bit-identical to those n calls (same lane mapping and summation order of the norm, the two scan bounds raised
 * the same way); the other 15 slots of a touched tile keep their bits, entries outside [0, ntotal) are skipped, ids are left alone.
 * When one row is named twice in a call, which of the two vectors it ends up holding is unspecified (lanes of different waves
 * write it unordered); every other row is unaffected.  rows: DEV int64 [n], x: DEV float32 [n,d]. */
int ivr_index_scatter(ivr_index *idx, const int64_t *rows /*DEV*/, const float *x /*DEV*/, int64_t n, int normalize,
                      ivr_stream stream);
/* faiss search_and_reconstruct(x, k): ivr_index_search_filtered (D and I bit-identical to it for the same arguments; filter NULL =
 * unfiltered) plus R: DEV float32 [nq,k,d], R[q,j] = the stored row that produced slot j, NaN rows for unused slots.  The row
 * positions come out of the final selection itself, so on an id-mapped index with duplicate labels R is the row that scored, not
 * the lowest row under its label.  Allocates nothing after ivr_index_reserve_search(max_nq, max_k), which also holds the nq x k
 * positions (8 bytes each). */
int ivr_index_search_reconstruct(ivr_index *idx, const float *q /*DEV*/, int nq, int k, int normalize_q, int64_t id_base,
                                 const ivr_id_filter *filter /*HOST, may be NULL*/, float *D /*DEV*/, int64_t *I /*DEV*/,
                                 float *R /*DEV*/, ivr_stream stream);

/* ---- inverted lists (faiss IndexIVFFlat) -------------------------------------------------------------
 * An inverted-file index is an ivr_index whose rows are ordered by list: list l is the run of rows [list_off[l], list_off[l + 1])
 * (list_off ascending, list_off[nlist] <= ntotal; the caller keeps the rows in that order, ivr_amd/ivf.py does it with gather +
 * add_with_ids).  ivr_index_search_lists is faiss search_preassigned: query i is scored against the rows of the lists
 * assign[i][0 .. p) only, and D / I are the top k of those rows under the contract of ivr_index_search (labels from the id table on
 * an id-mapped index, else the row number; unused slots -FLT_MAX / -1).  A score is the float32 inner product ivr_index_search
 * computes, to the bit; equal scores rank the lower row first, i.e. the lower list and inside a list the row stored first, whatever
 * the order of a row of assign.
 *   assign          DEV int64 [nq][p], EVERY ROW ASCENDING.  Entries outside [0, nlist) (-1, the empty slot of a coarse search,
 *                   included) are skipped; a list named twice in a row is scanned once (the two entries are adjacent).
 *   max_probe_rows  an upper bound of the rows any one query probes (the sum of its lists' sizes), e.g. the sum of the p longest
 *                   lists; clipped to ntotal.  It sizes the scratch: 8 bytes per probed row and query.  A query that probes more rows
 *                   than this bound returns no result at all (never a write outside the scratch).
 * The queries are worked off in chunks so that the scratch stays at 2^25 keys (256 MiB) or one query's max_probe_rows keys, whichever
 * is larger, plus 20 bytes per (query, list) pair of a chunk (at most 2^22 pairs).  Within a chunk a list is read once per 16 of the
 * queries that probe it.  Enqueue-only once the scratch has grown (a call that grows it allocates); not graph-capturable then. */
int ivr_index_search_lists(ivr_index *idx, const int64_t *list_off /*DEV [nlist+1]*/, int nlist, const float *q /*DEV [nq,d]*/, int nq,
                           const int64_t *assign /*DEV [nq][p]*/, int p, int64_t max_probe_rows, int k, int normalize_q,
                           float *D /*DEV [nq,k]*/, int64_t *I /*DEV [nq,k]*/, ivr_stream stream);
/* The centroid update of k-means: out[s] = the mean of rows[seg_off[s] .. seg_off[s + 1]) (row-major float32 [n,d]; seg_off ascending,
 * clipped to [0, n]), divided by its L2 norm when normalize (a zero mean stays zero).  Every column is summed in ascending row order
 * in double precision without atomics, so the result has the same bits on every run.  An empty segment gives a row of NaNs. */
int ivr_segment_mean(ivr_ctx *ctx, const float *rows /*DEV [n,d]*/, int64_t n, const int64_t *seg_off /*DEV [nseg+1]*/, int nseg, int d,
                     int normalize, float *out /*DEV [nseg,d]*/, ivr_stream stream);

/* ---- exact re-ranking of candidate lists (faiss IndexRefineFlat, IndexFlat::compute_distance_subset) ----
 * Query i is scored against the kc storage rows cand[i][0 .. kc) only: the rows a cheaper index (binary codes, inverted lists, a
 * graph) proposed.  The call is positional like ivr_index_gather, on plain and id-mapped indexes alike.  An entry outside
 * [0, ntotal), -1 included, is absent.  A score is the float32 inner product ivr_index_search reports for the same (query, row), to
 * the bit (the float32 tiles, the same summation order, -0.0 folded onto +0.0 as there); the bf16 scan copy is not read.
 *   D_all  DEV [nq][kc] or NULL: D_all[i][j] = the score of cand[i][j], -FLT_MAX for an absent entry.  Order and repeats are the
 *          caller's (compute_distance_subset).
 *   D, I   DEV [nq][k], both or neither, 1 <= k <= kc: the best k candidates of each query in the order of ivr_index_search, score
 *          descending and equal scores the lower row first, wherever they stood in cand.  I holds row positions.  A row named m
 *          times in one list appears m times, in adjacent slots (faiss does the same).  Slots beyond the present candidates hold
 *          -FLT_MAX / -1.
 * 1 <= kc <= IVR_MAX_K, nq >= 1, nq kc < 2^31 and at least one output, IVR_ERR_INVALID otherwise; an empty index gives absent
 * results only.  One wave scores 16 candidates of one query, so a single query's list spreads over the whole device; a random row
 * moves 16 times its bytes in cache lines, as for ivr_index_gather.  Scratch: 8 bytes per (query, candidate) when D / I are asked
 * for, grow-only.  Enqueue-only once the scratch has grown (a call that grows it allocates); not graph-capturable then. */
int ivr_index_rescore(ivr_index *idx, const float *q /*DEV [nq,d]*/, int nq, const int64_t *cand /*DEV [nq][kc]*/, int kc, int k,
                      int normalize_q, float *D_all /*DEV [nq][kc] or NULL*/, float *D /*DEV [nq][k] or NULL*/,
                      int64_t *I /*DEV [nq][k] or NULL*/, ivr_stream stream);

/* ---- clip search: sliding-window sequence match over the flat index ----------------------------------
 * Where in the stored rows does a run of L consecutive query frames occur?  The reference's TemporalAnalyzer.find_similar_sequences
 * (core.py:3644-3702) without its three Python loops.  q: DEV float32 [T,d] query frames, 1 <= L <= IVR_SEQ_MAX_LEN, T >= L.
 *   frame score   S[t, s] = the float32 inner product ivr_index_search reports for (query frame t, stored row s), to the bit
 *   window score  W[t, s] = (((S[t, s] + S[t+1, s+1]) + ...) + S[t+L-1, s+L-1]) / (float)L for target window t in [0, T - L] and start
 *                 row s in [0, ntotal - L]: L - 1 float32 additions in ascending order, each rounded on its own, then one correctly
 *                 rounded float32 division.  With unit rows and normalize_q that is the mean frame-wise cosine of the two runs.
 *   segments      seg_off: DEV int64 [nseg + 1], ascending, or NULL (then nseg is not read and the whole index is one segment).  A start
 *                 s is a candidate only when [s, s + L) lies inside one segment [seg_off[j], seg_off[j + 1]): a match never straddles
 *                 two videos.  Rows outside [seg_off[0], seg_off[nseg]) start nothing, empty segments are allowed, and fewer stored rows
 *                 than L give no candidate at all.
 * Both calls are positional like ivr_index_rescore and label a result with its start row, or with the stored id of that row on an
 * id-mapped index.  Scores are written as every search writes them (-0.0 as +0.0).
 *
 * ivr_index_search_sequences: D / I DEV [T - L + 1][k], per target window the k best starts by W, descending, equal scores the lower
 * start ROW first; unused slots (-FLT_MAX, -1).  1 <= k <= IVR_MAX_K.
 * ivr_index_range_search_sequences: every candidate with W >= threshold.  The test is >= because the reference's is (core.py:3687),
 * unlike the strict > of ivr_index_range_search.  Output as there: lims DEV int64 [T - L + 2], lims[0] = 0, the results of window t at
 * [lims[t], lims[t + 1]) in ascending start row; D / I DEV with room for `cap` entries, entries at positions >= cap are counted in
 * lims but not written (the caller re-calls with cap >= lims[T - L + 1]).  A NaN score matches nothing; a NaN threshold is
 * IVR_ERR_INVALID (+-inf are allowed).
 *
 * The windows are worked off in chunks.  Scratch on the index, grow-only: 8 bytes per (window of a chunk, start) with at most
 * IVR_SEQ_CHUNK_SLOTS slots per chunk (environment, read by ivr_index_create; default 2^25 = 256 MiB) or one window's ntotal - L + 1 when
 * that is more, and 4 bytes per (frame of a chunk rounded up to whole 16-frame tiles plus one tile, stored row).  The frames of
 * consecutive chunks overlap by L - 1 and are scored again.  The range call carries its running total from chunk to chunk on the
 * device.  Enqueue-only, no host synchronisation, once the scratch has grown (a call that grows it allocates); not graph-capturable
 * then. */
#define IVR_SEQ_MAX_LEN 64
int ivr_index_search_sequences(ivr_index *idx, const float *q /*DEV [T,d]*/, int T, int L, const int64_t *seg_off /*DEV [nseg+1] or NULL*/,
                               int nseg, int k, int normalize_q, float *D /*DEV [T-L+1,k]*/, int64_t *I /*DEV [T-L+1,k]*/, ivr_stream stream);
int ivr_index_range_search_sequences(ivr_index *idx, const float *q /*DEV [T,d]*/, int T, int L,
                                     const int64_t *seg_off /*DEV [nseg+1] or NULL*/, int nseg, float threshold, int normalize_q,
                                     int64_t *lims /*DEV [T-L+2]*/, float *D /*DEV [cap]*/, int64_t *I /*DEV [cap]*/, int64_t cap,
                                     ivr_stream stream);

/* ---- event search: chains of query events with bounded gaps over the flat index ------------------------
 * Where in the stored rows do m query events occur IN ORDER, not too far apart ("a door opens, THEN a dog jumps out, THEN the car drives
 * off")?  The gapped form of the clip search, which scores consecutive rows only.  q: DEV float32 [B][m][d], B >= 1 chains of
 * 1 <= m <= IVR_EVENT_MAX_LEN events each; 1 <= min_gap <= max_gap <= IVR_EVENT_MAX_GAP, in rows; ntotal < 2^31.
 *   frame score   S[j, r] = the float32 inner product ivr_index_search reports for (event j of the chain, stored row r), to the bit
 *   segments      seg_off as for the clip search: DEV int64 [nseg + 1], ascending, or NULL (nseg is not read, the index is one segment).
 *                 A row outside [seg_off[0], seg_off[nseg]) belongs to no segment and is no candidate of any step; empty segments are
 *                 allowed; a chain never leaves the segment of its end row
 *   step 0        C[0, r] = S[0, r] for every row inside a segment
 *   step j >= 1   the window of row r is [max(lo(r), r - max_gap), r - min_gap], lo(r) the start of r's segment.  No candidate of step
 *                 j - 1 in it: r is no candidate of step j.  Otherwise its predecessor P[j, r] is the candidate of the window with the
 *                 greatest C[j-1, .], -0.0 equal to +0.0, equal values the LOWER row (the order of every result key of the library), and
 *                 C[j, r] = (C[j-1, P[j, r]] + 0.0f) + S[j, r]: one float32 addition, rounded once
 *   chain score   W[r] = C[m-1, r] / (float)m of end row r: one correctly rounded division, written as every search writes scores
 *                 (-0.0 as +0.0).  Float32 addition is monotone, so C[m-1, r] is the maximum over ALL admissible chains that end in r of
 *                 the left-to-right sum ((S[0, r0] + 0 + S[1, r1]) + 0 + ...)
 *   path          r[m-1] = r, r[j-1] = P[j, r[j]]; reported in event order, as row numbers, or as stored ids on an id-mapped index
 * ivr_index_search_events: D DEV [B][k], I DEV [B][k][m]: per chain the k best end rows by W, descending, equal scores the lower END
 * row first, and the path behind each; unused slots -FLT_MAX and -1 in all m entries.  1 <= k <= IVR_MAX_K.
 * ivr_index_best_events_per_segment: D DEV [B][nseg], I DEV [B][nseg][m] (nseg = 1 without seg_off): for every segment its best end row
 * by the same order and its path, -FLT_MAX / -1 for a segment without a chain: which videos hold the sequence, all videos in one call.
 * Here B * nseg < 2^31.
 *
 * Launches per chunk of chains, all on `stream`, no host round trip: the score pass of the clip search over the chunk's frames; m - 1
 * step launches (a workgroup owns 1024 rows of one chain, holds the keys of the rows its windows reach in LDS and takes every window
 * maximum from block prefix / suffix maxima: the work per row does not grow with max_gap); the top-k selection or a key maximum per
 * segment; one backtrack launch that follows the stored 16-bit predecessor distances.  The segment bounds are one launch per call.
 * A chunk holds as many chains as IVR_SEQ_CHUNK_SLOTS / ntotal (one at least, 4096 / m at most).  Scratch on the index, grow-only:
 * per (chain of a chunk, stored row) 16 bytes of keys and 2 (m - 1) bytes of distances, 4 bytes per (frame of a chunk rounded up to
 * whole 16-frame tiles plus one tile, stored row) shared with the clip search, 8 bytes per stored row of segment bounds, 8 bytes per
 * result slot of a chunk.  m = 1 is ivr_index_search.  Enqueue-only, no host synchronisation, once the scratch has grown (a call that
 * grows it allocates); not graph-capturable then. */
#define IVR_EVENT_MAX_LEN 8
#define IVR_EVENT_MAX_GAP 4096
int ivr_index_search_events(ivr_index *idx, const float *q /*DEV [B,m,d]*/, int B, int m, int min_gap, int max_gap,
                            const int64_t *seg_off /*DEV [nseg+1] or NULL*/, int nseg, int k, int normalize_q, float *D /*DEV [B,k]*/,
                            int64_t *I /*DEV [B,k,m]*/, ivr_stream stream);
int ivr_index_best_events_per_segment(ivr_index *idx, const float *q /*DEV [B,m,d]*/, int B, int m, int min_gap, int max_gap,
                                      const int64_t *seg_off /*DEV [nseg+1] or NULL*/, int nseg, int normalize_q,
                                      float *D /*DEV [B,nseg]*/, int64_t *I /*DEV [B,nseg,m]*/, ivr_stream stream);

/* ---- grouped search: the best segments per query with their best rows -----------------------------------
 * Which VIDEOS answer a query, and with which frames?  Every other search ranks rows, and the keyframes of one shot fill the head of
 * such a list; vector stores call this grouping search (Milvus) or collapse with inner hits (Elasticsearch).  q: DEV float32 [nq,d].
 *   frame score   S[q, r] = the float32 inner product ivr_index_search reports for (query q, stored row r), to the bit
 *   row key       K[q, r] = (ordered S[q, r], ~r), the result key of every top-k of the library: the larger key ranks first, equal scores
 *                 the LOWER row, -0.0 equal to +0.0
 *   segments      seg_off as for the clip search: DEV int64 [nseg + 1], ascending, or NULL (nseg is not read, the index is one segment).
 *                 Empty segments are allowed and form no group; rows outside [seg_off[0], seg_off[nseg]) belong to no group; offsets
 *                 beyond ntotal are clipped
 *   group key     of segment j for query q: the greatest K[q, r] over the rows of j.  Groups rank by it, descending; among equal best
 *                 scores the segment that holds the lower best row comes first, which is the lower segment
 *   result        per query the best G groups, and within each the g best rows of that segment by K, descending
 * ivr_index_search_groups: Gseg DEV int64 [nq][G] the segment NUMBER of each chosen group; D DEV [nq][G][g] and I DEV [nq][G][g] the
 * scores and the rows, as row numbers, or as stored ids on an id-mapped index.  Unused group slots hold -1 in Gseg and -FLT_MAX / -1 in
 * all g entries; unused row slots of a short segment -FLT_MAX / -1.  1 <= G, 1 <= g <= IVR_GROUP_MAX_ROWS, G * g <= IVR_MAX_K, nq >= 1,
 * ntotal < 2^31; anything else is IVR_ERR_INVALID.  An empty index yields unused slots only.  Without seg_off, G = 1 and g = k is
 * ivr_index_search at k; with every row its own segment, G = k and g = 1 is ivr_index_search at k: both to the bit.
 * ivr_index_best_per_segment: D DEV [nq][nseg], I DEV [nq][nseg] (nseg = 1 without seg_off): the best row of EVERY segment and its
 * score, -FLT_MAX / -1 for an empty segment: the video-level score of every video in one call.  Here nq * nseg < 2^31.
 *
 * Launches, all on `stream`, no host round trip: the row -> segment table once per call; then per chunk of queries a fill of the
 * segment keys with 0 ("no row"), the segment-best pass (the score pass of the clip search, whose epilogue writes no score: it folds
 * the rows of a tile per segment in registers and issues one 64-bit atomic maximum per (query, segment touched) and wave), the top-G
 * selection over the segment keys (ivr_index_best_per_segment decodes them instead), a label pass, and for g > 1 the rows pass (one
 * workgroup per (query, group, piece of ivr_group_piece_rows() rows)) and its merge.  A maximum does not depend on the order of
 * arrival and the keys are unique: the same bits on every run and stream.  Scratch on the index, grow-only: 8 bytes per (query of a
 * chunk, segment), 4 bytes per stored row, 12 bytes per result slot (query of a chunk, group) and, for g > 1, 32 g bytes per (result
 * slot, piece; 16 pieces at most).  A chunk holds whole 16-query tiles, as many queries as keep the segment keys and the row lists
 * within IVR_SEQ_CHUNK_SLOTS slots each (16 at least, 4096 at most).  Enqueue-only, no host synchronisation, once the scratch has grown
 * (a call that grows it allocates); not graph-capturable then. */
#define IVR_GROUP_MAX_ROWS 64
int ivr_group_piece_rows(void);   /* stored rows one workgroup's piece of a long segment covers at least: tests size their cases from it */
int ivr_index_search_groups(ivr_index *idx, const float *q /*DEV [nq,d]*/, int nq, const int64_t *seg_off /*DEV [nseg+1] or NULL*/, int nseg,
                            int G, int g, int normalize_q, int64_t *Gseg /*DEV [nq,G]*/, float *D /*DEV [nq,G,g]*/,
                            int64_t *I /*DEV [nq,G,g]*/, ivr_stream stream);
int ivr_index_best_per_segment(ivr_index *idx, const float *q /*DEV [nq,d]*/, int nq, const int64_t *seg_off /*DEV [nseg+1] or NULL*/,
                               int nseg, int normalize_q, float *D /*DEV [nq,nseg]*/, int64_t *I /*DEV [nq,nseg]*/, ivr_stream stream);

/* ---- moment search: ranked time intervals per query ------------------------------------------------------
 * WHERE in a video does the query hold, and for how long?  A text query that matches a shot matches a run of adjacent keyframes: the
 * row searches fill their list with that run, the grouped search collapses it to the video.  A moment is the run itself, "video X,
 * frames 412 - 447", with its best frame: the scored form of the reference's unscored temporal_context (system.py:1967-1974).
 * q: DEV float32 [nq,d].
 *   frame score   S[q, r] = the float32 inner product ivr_index_search reports for (query q, stored row r), to the bit
 *   segments      seg_off as for the grouped search: DEV int64 [nseg + 1], ascending, or NULL (nseg is not read, the index is one
 *                 segment).  Empty segments are allowed; rows outside [seg_off[0], seg_off[nseg]) belong to nothing; offsets beyond
 *                 ntotal are clipped
 *   hot           row r is hot for q when it belongs to a segment and S[q, r] >= threshold (>=, as the clip search tests; a NaN score is
 *                 never hot)
 *   head          prev(r) = the greatest hot row below r.  A hot row is a head when prev(r) is none, lies in another segment, or
 *                 r - prev(r) > max_gap + 1: more than max_gap cold rows lie between them.  max_gap = 0: runs of consecutive hot rows
 *   moment        a head and the hot rows behind it up to the next head: lo = the head, hi = its last hot row (inclusive), cnt = its
 *                 hot rows, peak = its best hot row by (ordered S, ~row), the result key of every top-k of the library: score descending,
 *                 equal scores the LOWER row, -0.0 equal to +0.0
 * Per moment: D = S[q, peak] + 0.0f, I = the peak as a row number, or as its stored id on an id-mapped index; Lo, Hi and Cnt are
 * always row numbers and counts.
 * ivr_index_range_search_moments: every moment of every query in ascending lo, in the lims / cap contract of ivr_index_range_search:
 * lims DEV int64 [nq + 1], the moments of query i at positions lims[i] .. lims[i + 1]; entries at positions >= cap are counted and not
 * written.  D / I / Lo / Hi / Cnt DEV [cap] (never NULL, even for cap 0).
 * ivr_index_search_moments: per query the best k moments among those with cnt >= min_count, D / I / Lo / Hi / Cnt DEV [nq][k].
 * IVR_MOMENT_RANK_PEAK ranks by the peak key (equal scores: the lower peak row first), IVR_MOMENT_RANK_COUNT by cnt descending (equal
 * counts: the lower lo first).  Unused slots hold -FLT_MAX / -1 / -1 / -1 / 0.
 * nq >= 1, threshold not NaN, 0 <= max_gap <= 2^31 - 2, min_count >= 1, 1 <= k <= IVR_MAX_K, cap >= 0, nseg >= 1 with seg_off,
 * ntotal < 2^31; anything else is IVR_ERR_INVALID.  An empty index yields unused slots and lims of zeros.
 *
 * Launches, all on `stream`, no host round trip: the row -> segment table once per call; then per chunk of queries the score pass of
 * the clip search, a count pass (one workgroup per (query, block of ivr_moment_block_rows() rows): first hot row, last hot row and
 * the heads behind the first), a prefix pass per query (the prev every block enters with, the number of its first moment), the
 * totals (lims; the running total stays on the device from chunk to chunk), a fill of the chunk's moments with 0, the write pass (the
 * count pass's grid: every hot row learns its moment, a block folds each of its moments in LDS and contributes once per moment: plain
 * stores for a moment that lies inside the block, integer atomic maxima and sums for the two that may not), and the tail: a decode
 * pass (range), or the top-k selection over the rank keys and a gather.  Only integer maxima and sums cross workgroups, so the result
 * has the same bits on every run and stream; no launch waits on another workgroup.  The cost does not depend on max_gap.  Scratch on
 * the index, grow-only: 4 bytes per (query of a chunk, row), 16 per (query of a chunk, block), 24 per moment a chunk may hold (per
 * query min(ntotal, ntotal / (max_gap + 2) + nseg)), 12 per result slot.  A chunk holds whole 16-query tiles, as many queries as keep
 * the scores within IVR_SEQ_CHUNK_SLOTS floats (16 at least, 2048 at most).  Enqueue-only, no host synchronisation, once the scratch
 * has grown (a call that grows it allocates); not graph-capturable then. */
#define IVR_MOMENT_RANK_PEAK  0
#define IVR_MOMENT_RANK_COUNT 1
int ivr_moment_block_rows(void);   /* rows one workgroup of the run passes covers: tests size their cases from it */
int ivr_index_search_moments(ivr_index *idx, const float *q /*DEV [nq,d]*/, int nq, const int64_t *seg_off /*DEV [nseg+1] or NULL*/, int nseg,
                             float threshold, int max_gap, int min_count, int rank, int k, int normalize_q,
                             float *D /*DEV [nq,k]*/, int64_t *I /*DEV [nq,k]*/, int64_t *Lo, int64_t *Hi, int64_t *Cnt, ivr_stream stream);
int ivr_index_range_search_moments(ivr_index *idx, const float *q, int nq, const int64_t *seg_off, int nseg, float threshold, int max_gap,
                                   int normalize_q, int64_t *lims /*DEV [nq+1]*/, float *D /*DEV [cap]*/, int64_t *I, int64_t *Lo,
                                   int64_t *Hi, int64_t *Cnt, int64_t cap, ivr_stream stream);

/* ---- frame clustering: DBSCAN over the stored rows of the flat index ----------------------------------
 * Which stored frames are the same shot?  The reference's AdvancedKeyframeExtractor.cluster_similar_frames
 * (filter_research_update.py:113-134: sklearn DBSCAN on the precomputed 1 - cosine matrix) without the N x N matrix: a tiled self-join
 * of the storage, three passes, nothing stored per pair.
 *   score     S[q, r] = the float32 inner product ivr_index_search reports for (query = stored row q, stored row r), to the bit
 *   edge      rows i < j are neighbours iff both lie in one segment and (float)1 - S[j, i] <= eps: one rounded float32 subtraction, <=
 *             as sklearn's test.  Only S[j, i] with the HIGHER row as the query is read, so adjacency is symmetric by construction;
 *             S[i, i] is never read
 *   segments  seg_off: DEV int64 [nseg + 1], ascending, or NULL (then nseg is not read and the whole index is one segment), as for
 *             clip search: empty runs are allowed, rows outside [seg_off[0], seg_off[nseg]) belong to nothing (not core, label -1)
 *   core      row i is core iff 1 + (its neighbours) >= min_samples: a row always counts itself (sklearn reads the diagonal distance
 *             instead, which differs for a zero row or an eps below about 1e-6)
 *   cluster   a connected component of the core rows under edges; its root is its lowest row.  A non-core row with a core neighbour
 *             takes the cluster with the lowest root among its core neighbours (sklearn's result: it grows cluster 0 completely
 *             before it starts cluster 1); every other non-core row is noise
 *   labels    DEV int32 [ntotal]: the rank of the cluster's root among the roots of the row's own segment, ascending from 0 (numbering
 *             restarts in every segment), -1 for noise.  core: DEV uint8 [ntotal], 1 for a core row.  nclusters: DEV int32
 *             [max(nseg, 1)], the clusters of each segment (offsets clipped to [0, ntotal])
 * Positional like ivr_index_rescore, on plain and id-mapped indexes alike: labels are indexed by row.  eps negative or NaN,
 * min_samples < 1, ntotal >= 2^31 and NULL handles or outputs are IVR_ERR_INVALID; an empty index succeeds and writes nothing.
 * Every result is an integer built from integer atomic adds and minima: the same bits on every run.  Cost: three float32 self-join
 * passes over the pairs i < j of each segment.  Scratch on the index, grow-only: six 4-byte words per row.  Eight launches on the
 * caller's stream, no host synchronisation once the scratch has grown (a call that grows it allocates); not graph-capturable then. */
int ivr_index_dbscan(ivr_index *idx, float eps, int min_samples, const int64_t *seg_off /*DEV [nseg+1] or NULL*/, int nseg,
                     int32_t *labels /*DEV [ntotal]*/, uint8_t *core /*DEV [ntotal]*/, int32_t *nclusters /*DEV [max(nseg,1)]*/, ivr_stream stream);
/* The representative of each run of rows (filter_research_update.py:136-155): best[s] = the row of rows[seg_off[s] .. seg_off[s + 1])
 * (row-major float32 [n,d]; seg_off ascending, clipped to [0, n]) with the largest cosine to centers[s], as its position in `rows`, and
 * score[s] = that cosine, computed with the arithmetic of ivr_rowwise_cosine, to the bit (a zero norm counts as 1).  Equal cosines go to
 * the lower row, a NaN cosine is never the best, an empty run gives -1 / -FLT_MAX.  One workgroup per run. */
int ivr_segment_best_cosine(ivr_ctx *ctx, const float *rows /*DEV [n,d]*/, int64_t n, const int64_t *seg_off /*DEV [nseg+1]*/, int nseg, int d,
                            const float *centers /*DEV [nseg,d]*/, int64_t *best /*DEV [nseg]*/, float *score /*DEV [nseg]*/, ivr_stream stream);

/* ---- neighbour graph: segmented exact kNN self-join of the stored rows of the flat index --------------
 * For every stored row its k best OTHER rows of the same segment, optionally above a score: the reference's
 * MetadataManager._build_similarity_relationships (core.py:3493-3531: per folder the full cosine matrix, every row sorted, the top 10
 * others with cosine > 0.7) for all folders in one call, without a matrix and without copying a row into a query buffer.
 *   score       S[j, i] = the float32 inner product ivr_index_search / ivr_index_rescore report for (query = stored row j, stored row
 *               i), to the bit; every ordered pair is scored with its own j as the query
 *   segments    seg_off: DEV int64 [nseg + 1], ascending, or NULL (then nseg is not read and the whole index is one segment), as for
 *               ivr_index_dbscan: empty runs are allowed, rows outside [seg_off[0], seg_off[nseg]) have no neighbours and are nobody's
 *   candidates  of row j: the rows i != j of j's segment with i < ntotal whose S[j, i] is not NaN and, when threshold is not -inf,
 *               S[j, i] > threshold (strict, as the reference's > 0.7).  The row itself is left out by its number, not by its place in
 *               the order (the reference drops the first entry of its sort, which among duplicate frames may be another row)
 *   order       score descending, equal scores the lower row
 *   D           DEV float32 [ntotal][k], unused slots -FLT_MAX (a score of -0.0 is reported as +0.0, as by every top-k here)
 *   I           DEV int64 [ntotal][k]: ROW numbers, on plain and id-mapped indexes alike (as the labels of ivr_index_dbscan), unused -1
 *   count       DEV int32 [ntotal]: the used slots of each row
 * 1 <= k <= IVR_KNN_MAX_K; a NaN threshold, ntotal >= 2^31 and NULL handles or outputs are IVR_ERR_INVALID; an empty index succeeds
 * and writes nothing.  The candidates of a row are totally ordered by unique keys: the same bits on every run and stream.  Cost: one
 * float32 self-join pass over the ordered pairs of each segment.  Scratch on the index, grow-only: two words per row and at most 2^25
 * keys (256 MiB) of partial lists, an index too large for that is walked in chunks of rows.  One launch, then two per chunk, on the
 * caller's stream; no host synchronisation once the scratch has grown (a call that grows it allocates); not graph-capturable then. */
#define IVR_KNN_MAX_K 64
int ivr_knn_max_k(void);
int ivr_knn_piece_rows(void);   /* stored rows one workgroup's piece of a walk covers at least: tests size their cases from it */
int ivr_index_knn_graph(ivr_index *idx, int k, const int64_t *seg_off /*DEV [nseg+1] or NULL*/, int nseg, float threshold,
                        float *D /*DEV [ntotal][k]*/, int64_t *I /*DEV [ntotal][k]*/, int32_t *count /*DEV [ntotal]*/, ivr_stream stream);

/* ---- zero-shot tagging: the best labels of every stored row with their softmax probabilities, and of every segment ----------
 * CLIP's logits_per_image.softmax(dim=1) for the stored rows of the flat index against C label vectors (usually encoded texts): what
 * fills the reference's KeyframeMetadata.scene_tags (core.py:101, add_semantic_tags core.py:3278) without its remote vision call.
 *   labels      DEV float32 [C][d], 1 <= C <= IVR_TAG_MAX_LABELS; normalize: L2-normalised on the way in exactly as ivr_index_add does
 *   score       S[j, i] = the float32 inner product an ivr_index holding the labels reports for (query = stored row j, stored row =
 *               label i), to the bit
 *   candidates  of row j: the labels whose S[j, i] is not NaN (+-inf scores are outside the definition); order: score descending,
 *               equal scores the lower label
 *   probability P[j, i] = exp(scale (S[j, i] - m_j)) / Z_j with m_j the best score of the row and Z_j the sum of the numerators over
 *               ALL candidates, not only the listed ones.  exp is not reproducible to the bit elsewhere: P and Z lie within a stated
 *               relative bound of the float64 value (ivr_amd/tagging.py, tag_prob_bound) and have the same bits on every run and stream
 *   D, P, J     DEV float32 / float32 / int64 [ntotal][t]: score, probability and label number of the row's best t labels.  A slot is
 *               used while P >= min_prob (P descends with the rank, so min_prob truncates); unused slots hold -FLT_MAX / 0 / -1
 *   count, Z    DEV int32 / float32 [ntotal]: the used slots and Z_j (0 for a row without candidates)
 *   rows        only rows [row0, min(row1, ntotal)) are computed and written, at their own lines of the outputs
 * 1 <= t <= IVR_TAG_MAX_TOP.  IVR_ERR_INVALID: NULL handles, labels or outputs, C or t out of range, a scale that is not a positive
 * finite number, a NaN min_prob, row0 < 0 or row0 > row1, ntotal >= 2^31.  An empty index or range succeeds and writes nothing.
 * Cost: the stored rows of the range are read once, the label tiles once per block of up to 64 rows (from L2 / MALL).  Scratch on the
 * index, grow-only: the tiled labels.  Two launches on the caller's stream, no host synchronisation once the scratch has grown.
 *
 * ivr_index_tag_segments reduces the rows' lists per segment (seg_off as for ivr_index_knn_graph; NULL: one segment):
 *   votes[s][i] = the rows of segment s whose first label is i;  mass[s][i] = the sum over the rows of s and their used slots that
 *   name i of rint(P 2^24) as an integer.  Integer sums: the same bits whatever the order.  The result is the top g <= IVR_TAG_MAX_TOP
 *   labels of every segment by (mass or votes, per `rank`) descending, equal values the lower label, among the labels whose value is
 *   not 0: L DEV int64 [nseg][g] (unused -1), mass DEV uint64 [nseg][g], votes DEV int32 [nseg][g] (unused 0), rows DEV int32 [nseg]
 *   (the stored rows of each segment).  nseg x C may not exceed 2^25 table entries (IVR_ERR_INVALID beyond; 384 MiB of scratch at
 *   the limit); the row lists go through a scratch of at most 2^24 slots, a larger index is walked in chunks of rows.  An empty index
 *   succeeds and writes nothing. */
#define IVR_TAG_MAX_LABELS 4096
#define IVR_TAG_MAX_TOP 64
#define IVR_TAG_RANK_MASS 0
#define IVR_TAG_RANK_VOTES 1
int ivr_tag_max_labels(void);
int ivr_tag_max_top(void);
int ivr_index_tag_rows(ivr_index *idx, const float *labels /*DEV [C][d]*/, int C, int normalize, float scale, int t, float min_prob,
                       int64_t row0, int64_t row1, float *D /*DEV [ntotal][t]*/, float *P /*DEV [ntotal][t]*/, int64_t *J /*DEV [ntotal][t]*/,
                       int32_t *count /*DEV [ntotal]*/, float *Z /*DEV [ntotal]*/, ivr_stream stream);
int ivr_index_tag_segments(ivr_index *idx, const float *labels /*DEV [C][d]*/, int C, int normalize, float scale, int t, float min_prob,
                           const int64_t *seg_off /*DEV [nseg+1] or NULL*/, int nseg, int g, int rank, int64_t *L /*DEV [nseg][g]*/,
                           uint64_t *mass /*DEV [nseg][g]*/, int32_t *votes /*DEV [nseg][g]*/, int32_t *rows /*DEV [nseg]*/, ivr_stream stream);

/* ---- video search: stored videos ranked against a SET of query vectors ------------------------------------
 * Which stored videos look like this video or clip, whatever the order, frame rate or cut, and which contain all of these sub-queries
 * somewhere?  Every other member of the seg_off family takes one vector per query.  Here both sides hold several: the measure is the
 * two-sided reduction of the frame score matrix that vector stores ship for multi-vector documents as MaxSim / Chamfer similarity.
 *   frame score   S[i, r] = the float32 inner product ivr_index_search reports for (member i, stored row r), to the bit, -0.0 counted
 *                 as +0.0.  Precondition |S| <= 256; beyond it nothing faults and the result is unspecified
 *   sets          set_off: DEV int64 [nsets + 1], ascending: set s is the members [set_off[s], set_off[s + 1]) of q, 1 <= m_s <=
 *                 IVR_VIDEO_MAX_MEMBERS, 0 <= set_off[0], set_off[nsets] <= nq; NULL: all nq members are one set (nsets is not read).
 *                 It is read back once before the first launch: the one host synchronisation of a call
 *   videos        seg_off as for the grouped search: DEV int64 [nseg + 1], ascending, or NULL (one video); video j has the n_j rows of
 *                 [seg_off[j], seg_off[j + 1]) that are stored rows
 *   fix(t)        int64(rint(float32(t 2^24))): the fixed point of the tagging masses; the scaling is exact, so a term is rounded by at
 *                 most 2^-25
 *   Fsum[s, j]    the sum over the members i of s of fix(max over the rows r of j of S[i, r])
 *   Bsum[s, j]    the sum over the rows r of j of fix(max over the members i of s of S[i, r])
 *   V[s, j]       with F64 = double(Fsum) / (m_s 2^24) and B64 = double(Bsum) / (n_j 2^24): IVR_VIDEO_FORWARD float(F64) (MaxSim: "contains
 *                 all of these"), IVR_VIDEO_BACKWARD float(B64), IVR_VIDEO_SYMMETRIC float((F64 + B64) 0.5) (Chamfer).  An empty video
 *                 scores -FLT_MAX and is never ranked.  With m = 1, forward is the score of ivr_index_best_per_segment within 2^-25, not
 *                 to the bit
 *   order         videos rank by (V descending, video ascending) with the 64-bit key of every top-k of the library
 * ivr_index_video_scores: V DEV float32 [nsets][nseg] (nseg = 1 without seg_off).  Replaces ivr_index_best_per_segment over every member
 * plus ivr_index_tag_rows(t = 1) with the members as labels (whose IVR_TAG_MAX_LABELS caps the members of ALL sets together) plus a host
 * reduction per video: two float32 passes over the index and a join.
 * ivr_index_video_search: Vseg DEV int64 [nsets][k] and D DEV float32 [nsets][k], the k best videos of each set and their V; unused slots
 * -1 / -FLT_MAX.  exclude: DEV int64 [nsets] or NULL, one video left out per set (any value that is no video leaves none out).  Replaces
 * ivr_index_video_scores plus a top-k on the host.  1 <= k <= IVR_MAX_K.
 * An empty index yields -FLT_MAX / unused slots only.  IVR_ERR_INVALID: NULL handles, members or outputs, nq < 1, an empty or too large
 * set, a set_off that does not ascend or leaves [0, nq], nsets or nseg < 1 with their table, an unknown mode, k out of range,
 * ntotal >= 2^31.
 *
 * Launches, all on `stream`: the members tiled and re-tiled so that every set starts a 16-member tile; the row -> video table; then per
 * chunk of sets the score pass (a workgroup holds up to four member tiles of one set in LDS and streams 128 stored 16-row tiles past
 * them on the float32 MFMA; it writes no score, but one 32-bit atomic maximum per (member, video run, wave) and one store, or for a
 * set of more than one block one atomic maximum, per (row, block)), the two reductions (integer atomic adds only), the finish in
 * float64 and the top-k selection.  Maxima and integer sums do not depend on the order of arrival: the same bits on every run and
 * stream.  Scratch on the index, grow-only: 4 bytes per (member of a chunk, video) and per (set of a chunk, stored row), 24 bytes per
 * (set of a chunk, video), two copies of the members.  A chunk holds as many whole sets as keep each table within
 * IVR_SEQ_CHUNK_SLOTS slots, one at least.  Not graph-capturable (the read-back). */
#define IVR_VIDEO_MAX_MEMBERS 4096
#define IVR_VIDEO_FORWARD 0
#define IVR_VIDEO_BACKWARD 1
#define IVR_VIDEO_SYMMETRIC 2
int ivr_index_video_scores(ivr_index *idx, const float *q /*DEV [nq,d]*/, int nq, const int64_t *set_off /*DEV [nsets+1] or NULL*/, int nsets,
                           const int64_t *seg_off /*DEV [nseg+1] or NULL*/, int nseg, int mode, int normalize_q,
                           float *V /*DEV [nsets][nseg]*/, ivr_stream stream);
int ivr_index_video_search(ivr_index *idx, const float *q /*DEV [nq,d]*/, int nq, const int64_t *set_off /*DEV [nsets+1] or NULL*/, int nsets,
                           const int64_t *seg_off /*DEV [nseg+1] or NULL*/, int nseg, int mode, int normalize_q, int k,
                           const int64_t *exclude /*DEV [nsets] or NULL*/, int64_t *Vseg /*DEV [nsets][k]*/, float *D /*DEV [nsets][k]*/,
                           ivr_stream stream);

/* ---- binary codes (faiss IndexBinaryFlat, and the sign-bit encoder of IndexLSH) --------------------------
 * Stands in for faiss.IndexLSH(dimension, 256), one of the index types of _create_index (core.py:1198-1230): a row is stored as
 * nbits sign bits (32 bytes at 256 bits, where the flat index stores 2-4.6 KB) and ranked by Hamming distance.
 * A code is code_size = (nbits + 7) / 8 caller-facing bytes in faiss order: bit j of a code is bit j & 7 of byte j >> 3
 * (numpy.packbits(..., bitorder="little")).  The bits of the last byte at or above nbits are pad bits: they are ignored in stored
 * codes and in query codes alike, and ivr_bin_index_get_codes returns them as 0.  On the device a code is padded with zeros to whole
 * 16-byte words and the rows are interleaved per 64, so that one lane reads one row with 16-byte loads and a wave reads 1 KiB
 * contiguous per load ("binary codes").  The allocation grows like ivr_index's; capacity below 2^31 rows. */
typedef struct ivr_bin_index ivr_bin_index;
#define IVR_BIN_MAX_BITS 2048
int ivr_bin_index_create(ivr_ctx *ctx, int nbits, int64_t capacity_rows, ivr_bin_index **out);   /* 1 <= nbits <= IVR_BIN_MAX_BITS */
int ivr_bin_index_destroy(ivr_bin_index *idx);
int ivr_bin_index_reset(ivr_bin_index *idx);                /* ntotal = 0 */
int64_t ivr_bin_index_ntotal(ivr_bin_index *idx);
int ivr_bin_index_block_rows(void);     /* rows per workgroup block of the search passes: tests size their cases from it */
/* append n codes; grows the allocation when the capacity is exceeded (a call that grows synchronises the device) */
int ivr_bin_index_add(ivr_bin_index *idx, const uint8_t *codes /*DEV [n][code_size]*/, int64_t n, ivr_stream stream);
/* codes of rows [start, start + n) as they were added (pad bits 0); start + n <= ntotal */
int ivr_bin_index_get_codes(ivr_bin_index *idx, int64_t start, int64_t n, uint8_t *out /*DEV [n][code_size]*/, ivr_stream stream);
/* Exact top k by Hamming distance: D ascending, equal distances rank the lower row first, unused slots (k > ntotal, empty index)
 * hold INT32_MAX in D and -1 in I, as faiss's integer heap leaves them.  1 <= k <= IVR_MAX_K, nq >= 1.  The top k is selected by
 * counting (histogram of distances per query, threshold distance, ranks by prefix sums: no float compares, no cursor atomics, the
 * same rows on every run).  Scratch: 16-byte-padded queries, and per chunk of at most 64 queries 4 (nbits + 1) + 8 ntotal / 64 + 8 k
 * bytes per query; nothing is written per (query, row) pair.  Enqueue-only once the scratch has grown (a call that grows it
 * allocates and cannot be captured into a hipGraph). */
int ivr_bin_index_search(ivr_bin_index *idx, const uint8_t *qcodes /*DEV [nq][code_size]*/, int nq, int k, int32_t *D /*DEV [nq][k]*/,
                         int64_t *I /*DEV [nq][k]*/, ivr_stream stream);
/* faiss IndexLSH's encoder: proj[i][j] = <x[i], rot[j]> accumulated in float32 on the float32 MFMA in a fixed order (no atomics:
 * the same input gives the same bits on every run); rot == NULL: proj[i][j] = x[i][j], which needs nbits <= d (faiss's "first nbits
 * coordinates").  Bit j of code i is set iff proj[i][j] - thr[j] >= 0.0f (thr == NULL: 0; faiss fvecs2bitvecs after the threshold
 * subtraction); pad bits are written as 0.  proj != NULL also receives the float32 projections, before the threshold (threshold
 * training reads them).  x: DEV float32 [n][d], 1 <= d <= 65536; n == 0 is a no-op. */
int ivr_sign_encode(ivr_ctx *ctx, const float *x /*DEV [n][d]*/, int64_t n, int d, const float *rot /*DEV [nbits][d] or NULL*/,
                    const float *thr /*DEV [nbits] or NULL*/, int nbits, uint8_t *codes /*DEV [n][code_size]*/,
                    float *proj /*DEV [n][nbits] or NULL*/, ivr_stream stream);

/* ---- product quantisation (faiss IndexPQ) ---------------------------------------------------------------------
 * The reference's _create_index never builds an IndexPQ; it is here as the compressed base of the re-ranking index: a row is stored
 * as M bytes, byte m naming one of the 256 centroids of the codebook of slice m (floats m dsub .. (m + 1) dsub of the row, dsub =
 * d / M), and ranked by a sum of M table lookups (asymmetric inner product).  codebooks: DEV float32 [M][256][dsub].  The codes live
 * in an ivr_bin_index of 8 M bits (ivr_bin_index_create / _add / _get_codes / _reset as they are), so one lane reads one row with
 * 16-byte loads ("product quantisation").  1 <= M <= IVR_PQ_MAX_M and d % M == 0, IVR_ERR_INVALID otherwise. */
#define IVR_PQ_MAX_M 128
/* codes[i][m] = the j in [0, 256) that minimises |slice m of x[i] - codebooks[m][j]|^2, the lower j on equal distances.  The
 * distance is evaluated in float32 as |c|^2 - 2 <x, c> (the norm of x is common to all j), each sum in ascending coordinate order:
 * two centroids with the same bits get the same distance, and a code is within the float32 rounding of the evaluation of the true
 * argmin (pq_encode_ref of ivr_amd/pq.py states the bound).  A slice's codebook is held in LDS for dsub <= 64; wider slices read it
 * through the caches (slow, no limit on dsub).  x: DEV float32 [n][d], 1 <= d <= 65536; n == 0 is a no-op.  Enqueue-only. */
int ivr_pq_encode(ivr_ctx *ctx, const float *x /*DEV [n][d]*/, int64_t n, int d, const float *codebooks /*DEV [M][256][dsub]*/, int M,
                  uint8_t *codes /*DEV [n][M]*/, ivr_stream stream);
/* T[i][m][j] = <slice m of q[i], codebooks[m][j]>, accumulated in float32 in ascending coordinate order from zero (no atomics: the
 * same bits on every run).  nq >= 1.  Enqueue-only. */
int ivr_pq_tables(ivr_ctx *ctx, const float *q /*DEV [nq][d]*/, int nq, int d, const float *codebooks /*DEV [M][256][dsub]*/, int M,
                  float *T /*DEV [nq][M][256]*/, ivr_stream stream);
/* Table-lookup top k over the codes of an index created with nbits = 8 M.  The score of row r for query i is
 * (((T[i][0][c0] + T[i][1][c1]) + T[i][2][c2]) + ...), c = the code of r: plain float32 additions in ascending m, so the bits are
 * those of the same loop on a CPU.  D / I under the contract of ivr_index_search: score descending (-0.0 counts and is reported as
 * +0.0), equal scores the lower row first, I the row number, unused slots (k > ntotal, empty index) -FLT_MAX / -1.  Exact: the best
 * score of every 64-row group is written, the best k groups are selected, their rows re-scored into 64-bit keys and the best k keys
 * selected (the top k rows lie in the top k groups by (best score, lower group)).  T: DEV float32 [nq][M][256], 16-byte aligned,
 * finite.  1 <= k <= IVR_MAX_K, nq >= 1.  A workgroup keeps the tables of 128 / M queries (1 .. 8) in LDS and reads each code word
 * once for all of them.  Scratch per chunk of queries (at most 4096, fewer when k or the index is large): 4 bytes per (query, 64-row
 * group) and 520 bytes per (query, selected group), grow-only.  Enqueue-only once the scratch has grown (a call that grows it
 * allocates and cannot be captured into a hipGraph). */
int ivr_bin_index_search_pq(ivr_bin_index *idx, const float *T /*DEV [nq][M][256]*/, int nq, int M, int k, float *D /*DEV [nq][k]*/,
                            int64_t *I /*DEV [nq][k]*/, ivr_stream stream);

/* ---- inverted lists over product-quantised codes (faiss IndexIVFPQ, inner product) ---------------------------------
 * The coarse quantizer of the inverted-file index joined with the codes of the product quantiser ("inverted
 * lists over PQ codes"; the definitions are the numpy functions ivfpq_pack_ref, ivfpq_unpack_ref and ivfpq_scan_ref of
 * ivr_amd/ivfpq.py).  The object stores M-byte codes ordered by list, every list padded to whole 64-row groups in the interleaved
 * layout of ivr_bin_index (pad bytes and pad rows zero), and the int64 label of every packed position (-1 on a pad row).  Training,
 * the coarse assignment and the encoding of residuals are the caller's (ivr_pq_encode, ivr_pq_tables as they are).  Packed positions,
 * pads included, stay below 2^32.  One stream at a time per handle. */
typedef struct ivr_ivfpq ivr_ivfpq;
int ivr_ivfpq_create(ivr_ctx *ctx, int M, int nlist, ivr_ivfpq **out);     /* 1 <= M <= IVR_PQ_MAX_M, nlist >= 1; holds no rows */
int ivr_ivfpq_destroy(ivr_ivfpq *idx);
int ivr_ivfpq_reset(ivr_ivfpq *idx);                         /* ntotal = 0, every list empty */
int64_t ivr_ivfpq_ntotal(ivr_ivfpq *idx);
int ivr_ivfpq_probe_queries(void);      /* queries per workgroup of the probe-table kernel (the scan takes one query per workgroup):
                                           tests size their cases from it */
/* Replace the content: n rows ordered by list, list l = rows [list_off[l], list_off[l + 1]) with list_off[0] = 0 and list_off[nlist]
 * = n (IVR_ERR_INVALID otherwise, and for more than 2^32 packed positions).  Every label must be >= 0: a negative one marks a pad
 * row, and a row stored under it is left out of every search (the labels live on the device and are not checked here).  list_off is
 * read on the HOST during the call; codes and ids are packed by one kernel on `stream` and may be released once it has run.  When the
 * call fails after its arguments were accepted (allocation, copy or launch), the object is left empty.  Synchronises the device first (a search in flight
 * still reads the old lists) and allocates when the content outgrows the buffers. */
int ivr_ivfpq_set_lists(ivr_ivfpq *idx, const uint8_t *codes /*DEV [n][M]*/, const int64_t *ids /*DEV [n]*/,
                        const int64_t *list_off /*HOST [nlist + 1]*/, int64_t n, ivr_stream stream);
/* the codes and / or labels of the list-ordered rows [start, start + n) as they were set; start + n <= ntotal */
int ivr_ivfpq_get_codes(ivr_ivfpq *idx, int64_t start, int64_t n, uint8_t *codes /*DEV [n][M] or NULL*/, int64_t *ids /*DEV [n] or NULL*/,
                        ivr_stream stream);
/* Table-lookup top k over the lists each query probes.  assign[i] names the lists of query i in ASCENDING order: an entry outside
 * [0, nlist) is skipped, a list named twice (adjacent entries) counts once, with the coarse score of its first entry.  The score of a
 * row with code c in the list of entry j is (((coarse[i][j] + T[i][0][c0]) + T[i][1][c1]) + ...): plain float32 additions, coarse
 * first, then ascending m (coarse == NULL: +0.0).  D / I under the contract of ivr_index_search: score descending (-0.0 counts and is
 * reported as +0.0), equal scores the row in the lower list first and inside a list the row set earlier, I the row's label, unused
 * slots -FLT_MAX / -1.  T: DEV float32 [nq][M][256], 16-byte aligned, finite.  1 <= k <= IVR_MAX_K, nq >= 1, p >= 1.  Per chunk of
 * queries three launches on `stream`, no host round trip: the probe table (one wave per query), the scan (a workgroup of 8 waves
 * keeps ONE query's table in LDS, M KiB, and scores a share of the 64-row groups of that query's lists into 64-bit keys) and
 * select_topk.  Scratch per chunk (at most 2^25 key slots, one query's at least): 8 bytes per row, pads included, of the p longest
 * lists per query, and 4 p + 4 bytes per query; grow-only.  Enqueue-only once the scratch has grown (a call that grows it allocates
 * and cannot be captured into a hipGraph). */
int ivr_ivfpq_search(ivr_ivfpq *idx, const float *T /*DEV [nq][M][256]*/, const float *coarse /*DEV [nq][p] or NULL*/,
                     const int64_t *assign /*DEV [nq][p]*/, int nq, int p, int k, float *D /*DEV [nq][k]*/, int64_t *I /*DEV [nq][k]*/,
                     ivr_stream stream);

/* ---- scalar quantisation (faiss IndexScalarQuantizer, QT_8bit, inner product) ------------------------------------
 * The reference's _create_index never builds an IndexScalarQuantizer; it is here as the compressed base between the flat index and
 * the 32 - 64 byte codes: a row is stored as d bytes, byte j = the bucket of coordinate j between vmin[j] and vmin[j] + vdiff[j], and
 * ranked by an exact integer inner product on the int8 MFMA ("scalar quantisation"; the definitions are the
 * numpy functions sq_encode_ref, sq_query_ref and sq_scan_ref of ivr_amd/sq.py).  1 <= d <= 1024, IVR_ERR_INVALID otherwise: the
 * bound keeps 16256 * 128 * d inside the int32 accumulator. */
/* codes[i][j] = min(255, int(255 * xi)), xi = clamp((x[i][j] - vmin[j]) / vdiff[j], 0, 1) and 0 where vdiff[j] == 0: faiss's
 * Codec8bit, every operation one float32 rounding (correctly rounded division, no fused multiply-add), truncating.  x must be
 * finite: what a NaN encodes to is unspecified.  n == 0 is a no-op.  Enqueue-only. */
int ivr_sq_encode(ivr_ctx *ctx, const float *x /*DEV [n][d]*/, int64_t n, int d, const float *vmin /*DEV [d]*/,
                  const float *vdiff /*DEV [d]*/, uint8_t *codes /*DEV [n][d]*/, ivr_stream stream);
/* The integer form of a batch of queries.  With w[j] = q[j] * gain[j] and m = max |w[j]|: scale = m / 16256 (1 when m == 0),
 * t[j] = clamp(rint(w[j] / scale), -16256, 16256) (float32 division, rounding half to even), bias = sum q[j] * offset[j] in float32
 * (within (d + 2) 2^-24 sum |q[j] offset[j]| of the exact sum).  t and scale carry the bits of sq_query_ref.  q must be finite.
 * nq >= 1.  Enqueue-only. */
int ivr_sq_query(ivr_ctx *ctx, const float *q /*DEV [nq][d]*/, int nq, int d, const float *gain /*DEV [d]*/,
                 const float *offset /*DEV [d]*/, int16_t *t /*DEV [nq][d]*/, float *scale /*DEV [nq]*/, float *bias /*DEV [nq]*/,
                 ivr_stream stream);
/* The stored codes: signed c' = code - 128, K padded with zeros to a multiple of 64, tiled per 16 rows so that one wave-wide 16-byte
 * load is 1 KiB contiguous and is the A operand of one v_mfma_i32_16x16x64_i8.  Rows are allocated by the first add, in whole 64-row
 * groups; capacity below 2^31 rows. */
typedef struct ivr_sq_index ivr_sq_index;
int ivr_sq_index_create(ivr_ctx *ctx, int d, ivr_sq_index **out);
int ivr_sq_index_destroy(ivr_sq_index *idx);                /* IVR_ERR_INVALID for NULL, as every entry of this section */
int ivr_sq_index_reset(ivr_sq_index *idx);                  /* ntotal = 0; the bytes stay and are never read as rows */
int64_t ivr_sq_index_ntotal(ivr_sq_index *idx);             /* -1 for NULL */
/* append n codes as ivr_sq_encode makes them (unsigned); writes the new rows only */
int ivr_sq_index_add(ivr_sq_index *idx, const uint8_t *codes /*DEV [n][d]*/, int64_t n, ivr_stream stream);
/* codes of rows [start, start + n) as they were added; start + n <= ntotal */
int ivr_sq_index_get_codes(ivr_sq_index *idx, int64_t start, int64_t n, uint8_t *out /*DEV [n][d]*/, ivr_stream stream);
/* Integer top k.  acc of row r for query i = sum_j t[i][j] * c'[r][j], exact in int32 (t as ivr_sq_query makes it; a |t| beyond 16256
 * is clamped to it).  Rows are ranked by (acc descending, row ascending): integers only.  D = float(acc) * scale[i] + bias[i]: one
 * conversion to nearest-even, one float32 multiplication, one float32 addition; I the row number; unused slots (k > ntotal, empty
 * index) -FLT_MAX / -1.  Exact: the best acc of every 64-row group is written, the best k groups are selected, their rows re-scored
 * into 64-bit keys (acc ^ 0x80000000) << 32 | ~row and the best k keys selected.  1 <= k <= IVR_MAX_K, nq >= 1.  The index is read
 * once per 32 queries.  Scratch: 2 ceil(d / 64) 64 bytes per query, and per chunk of queries (at most 4096, fewer when k or the
 * index is large) 4 bytes per (query, 64-row group) and 520 bytes per (query, selected group), grow-only.  Enqueue-only once the
 * scratch has grown (a call that grows it allocates and cannot be captured into a hipGraph). */
int ivr_sq_index_search(ivr_sq_index *idx, const int16_t *t /*DEV [nq][d]*/, const float *scale /*DEV [nq]*/,
                        const float *bias /*DEV [nq]*/, int nq, int k, float *D /*DEV [nq][k]*/, int64_t *I /*DEV [nq][k]*/,
                        ivr_stream stream);

/* ---- inverted lists over scalar-quantiser codes (faiss IndexIVFScalarQuantizer, QT_8bit, inner product) -----------------
 * The coarse quantizer of the inverted-file index joined with the codes of the scalar quantiser ("inverted
 * lists over SQ codes"; the definitions are the numpy functions ivfsq_pack_ref, ivfsq_unpack_ref and ivfsq_scan_ref of
 * ivr_amd/ivfsq.py).  The object mirrors ivr_ivfpq entry for entry.  It stores d-byte codes ordered by list, every list padded to
 * whole 64-row groups; over the packed positions (64 goff[l] + i for row i of list l, goff = the groups in front of the list) the
 * layout is that of ivr_sq_index: signed c' = code - 128, K padded with zeros to a multiple of 64, tiled per 16 positions (pad bytes
 * and pad rows zero), and the int64 label of every packed position (-1 on a pad row).  Training, the coarse assignment, the encoding
 * of residuals and the integer form of the queries are the caller's (ivr_sq_encode, ivr_sq_query as they are).  Packed positions,
 * pads included, stay below 2^32.  One stream at a time per handle. */
#define IVR_SQ_MAX_D 1024
typedef struct ivr_ivfsq ivr_ivfsq;
int ivr_ivfsq_create(ivr_ctx *ctx, int d, int nlist, ivr_ivfsq **out);     /* 1 <= d <= IVR_SQ_MAX_D, nlist >= 1; holds no rows */
int ivr_ivfsq_destroy(ivr_ivfsq *idx);
int ivr_ivfsq_reset(ivr_ivfsq *idx);                         /* ntotal = 0, every list empty */
int64_t ivr_ivfsq_ntotal(ivr_ivfsq *idx);
/* Replace the content: n rows ordered by list, list l = rows [list_off[l], list_off[l + 1]) with list_off[0] = 0 and list_off[nlist]
 * = n (IVR_ERR_INVALID otherwise, and for more than 2^32 packed positions).  codes as ivr_sq_encode makes them (unsigned).  Every
 * label must be >= 0 (the labels live on the device and are not checked here).  list_off is read on the HOST during the call; codes
 * and ids are packed by one kernel on `stream` and may be released once it has run.  When the call fails after its arguments were
 * accepted (allocation, copy or launch), the object is left empty.  Synchronises the device first (a search in flight still reads the
 * old lists) and allocates when the content outgrows the buffers. */
int ivr_ivfsq_set_lists(ivr_ivfsq *idx, const uint8_t *codes /*DEV [n][d]*/, const int64_t *ids /*DEV [n]*/,
                        const int64_t *list_off /*HOST [nlist + 1]*/, int64_t n, ivr_stream stream);
/* the codes and / or labels of the list-ordered rows [start, start + n) as they were set; start + n <= ntotal */
int ivr_ivfsq_get_codes(ivr_ivfsq *idx, int64_t start, int64_t n, uint8_t *codes /*DEV [n][d] or NULL*/, int64_t *ids /*DEV [n] or NULL*/,
                        ivr_stream stream);
/* Integer-scored top k over the lists each query probes.  assign[i] names the lists of query i in ASCENDING order: an entry outside
 * [0, nlist) is skipped, a list named twice (adjacent entries) counts once, with the coarse score of its first entry.  For a row with
 * stored bytes c' in the list of entry j, acc = sum_m t[i][m] * c'[m] exact in int32 (t as ivr_sq_query makes it; a |t| beyond 16256
 * is clamped to it) and D = ((float(acc) * scale[i]) + bias[i]) + coarse[i][j]: one conversion to nearest-even, one float32
 * multiplication and two float32 additions in this order, no fused multiply-add (coarse == NULL: +0.0).  D / I under the contract of
 * ivr_index_search: D descending (-0.0 counts and is reported as +0.0), equal D the row in the lower list first and inside a list the
 * row set earlier, I the row's label, unused slots -FLT_MAX / -1.  1 <= k <= IVR_MAX_K, nq >= 1, p >= 1.  The queries are staged
 * once per call into their two int8 halves; then per chunk of queries, on `stream` and without a host round trip: the probe tables
 * of ivr_index_search_lists (pairs grouped by list, 16-query pair tiles, one key slot per probed row), the list scan (a workgroup per
 * (pair tile, 256-row split) gathers both halves of its up to 16 queries into LDS, 2 KiB per 64 coordinates, and reads every 16-row
 * tile of its split once for two v_mfma_i32_16x16x64_i8 per K step) and select_topk.  Scratch: 2 ceil(d / 64) 64 bytes per query, and
 * per chunk (at most 2^25 key slots, one query's at least, and 2^22 pairs) 8 bytes per row of the p longest lists per query and
 * 20 p + 8 bytes per query; grow-only.  Enqueue-only once the scratch has grown (a call that grows it allocates and cannot be
 * captured into a hipGraph). */
int ivr_ivfsq_search(ivr_ivfsq *idx, const int16_t *t /*DEV [nq][d]*/, const float *scale /*DEV [nq]*/, const float *bias /*DEV [nq]*/,
                     const float *coarse /*DEV [nq][p] or NULL*/, const int64_t *assign /*DEV [nq][p]*/, int nq, int p, int k,
                     float *D /*DEV [nq][k]*/, int64_t *I /*DEV [nq][k]*/, ivr_stream stream);

/* ---- 4-bit product quantisation (faiss IndexPQFastScan, inner product) --------------------------------------------------
 * M sub-quantizers of 16 centroids each: a row is M / 2 bytes, byte j = code[2 j] | code[2 j + 1] << 4 (faiss's packing), and is
 * ranked by a sum of M lookups in 16-entry tables of 8-bit values that the scan holds in registers ("4-bit
 * product quantisation"; the definitions are the numpy functions pqfs_encode_ref, pqfs_tables_ref, pqfs_quantize_ref and
 * pqfs_scan_ref of ivr_amd/pqfs.py).  M even, 2 <= M <= IVR_PQFS_MAX_M, d % M == 0, IVR_ERR_INVALID otherwise: 255 M fits the
 * unsigned 16-bit accumulator of the scan.  centroids: DEV float32 [M][16][d / M]. */
#define IVR_PQFS_MAX_M 256
int ivr_pqfs_pass_queries(void);        /* queries that share one pass over the stored codes */
/* codes[i][j] = c(2 j) | c(2 j + 1) << 4 with c(m) the centroid of slice m nearest to slice m of x[i]: sum_t (x_t - c_t)^2 in float32,
 * ascending t, equal distances the lower centroid (pqfs_encode_ref states the tolerance).  n == 0 is a no-op.  Enqueue-only. */
int ivr_pqfs_encode(ivr_ctx *ctx, const float *x /*DEV [n][d]*/, int64_t n, int d, const float *centroids, int M,
                    uint8_t *codes /*DEV [n][M / 2]*/, ivr_stream stream);
/* The tables of a batch of queries in one call.  T[i][m][j] = <slice m of q[i], centroids[m][j]>, float32 from zero in ascending
 * coordinate order (within (d / M + 2) 2^-24 sum |q_t c_t| of the exact sum); written when T != NULL.  From those floats, every
 * step one float32 rounding and no fused multiply-add: lo[m] = min_j T[m][j], span = max_m (max_j T[m][j] - lo[m]), a = 255 / span,
 * U[m][j] = clamp(rint((T[m][j] - lo[m]) * a), 0, 255) (ties to even), scale = span / 255, bias = ((lo[0] + lo[1]) + ...) in
 * ascending m; a = 0, U = 0 and scale = 0 when span == 0 or 255 / span is not finite.  q must be finite.  nq >= 1.  Enqueue-only. */
int ivr_pqfs_tables(ivr_ctx *ctx, const float *q /*DEV [nq][d]*/, int nq, int d, const float *centroids, int M,
                    float *T /*DEV [nq][M][16] or NULL*/, uint8_t *U /*DEV [nq][M][16]*/, float *scale /*DEV [nq]*/,
                    float *bias /*DEV [nq]*/, ivr_stream stream);
/* the quantiser of ivr_pqfs_tables alone, on caller-supplied finite float tables */
int ivr_pqfs_quantize(ivr_ctx *ctx, const float *T /*DEV [nq][M][16]*/, int nq, int M, uint8_t *U /*DEV [nq][M][16]*/,
                      float *scale /*DEV [nq]*/, float *bias /*DEV [nq]*/, ivr_stream stream);
/* The stored codes, per block of 256 rows: lane l of a wave holds rows l, l + 64, l + 128 and l + 192, dword j of the lane is byte j
 * of those four rows, and 8 sub-quantizers (4 dwords) are one 16-byte word per lane, 1 KiB contiguous per wave; the sub-quantizers
 * behind M hold code 0.  Rows are allocated by the first add, in whole blocks; capacity below 2^31 rows. */
typedef struct ivr_pqfs_index ivr_pqfs_index;
int ivr_pqfs_index_create(ivr_ctx *ctx, int M, ivr_pqfs_index **out);
int ivr_pqfs_index_destroy(ivr_pqfs_index *idx);            /* IVR_ERR_INVALID for NULL, as every entry of this section */
int ivr_pqfs_index_reset(ivr_pqfs_index *idx);              /* ntotal = 0; the bytes stay and are never read as rows */
int64_t ivr_pqfs_index_ntotal(ivr_pqfs_index *idx);         /* -1 for NULL */
/* append n codes as ivr_pqfs_encode makes them; writes the new rows only */
int ivr_pqfs_index_add(ivr_pqfs_index *idx, const uint8_t *codes /*DEV [n][M / 2]*/, int64_t n, ivr_stream stream);
/* codes of rows [start, start + n) as they were added; start + n <= ntotal */
int ivr_pqfs_index_get_codes(ivr_pqfs_index *idx, int64_t start, int64_t n, uint8_t *out /*DEV [n][M / 2]*/, ivr_stream stream);
/* Integer top k.  acc of row r for query i = sum_m U[i][m][code[r][m]], exact (at most 255 M <= 65280).  Rows are ranked by (acc
 * descending, row ascending): integers only.  D = float(acc) * scale[i] + bias[i]: one conversion, one float32 multiplication, one
 * float32 addition; I the row number; unused slots (k > ntotal, empty index) -FLT_MAX / -1.  Exact: the best acc of every 64-row
 * group is written, the best k groups are selected, their rows re-scored into 64-bit keys (acc ^ 0x80000000) << 32 | ~row and the
 * best k keys selected.  U 16-byte aligned.  1 <= k <= IVR_MAX_K, nq >= 1.  The codes are read once per ivr_pqfs_pass_queries()
 * queries; a table reaches the lookups through a wave-uniform (scalar) load, and a lookup of four rows is two v_perm_b32 and a
 * v_bfi_b32.  Scratch: 128 ceil(M / 8) bytes per query, and per chunk of queries (at most 4096, fewer when k or the index is large)
 * 4 bytes per (query, 64-row group) and 520 bytes per (query, selected group), grow-only.  Enqueue-only once the scratch has grown
 * (a call that grows it allocates and cannot be captured into a hipGraph). */
int ivr_pqfs_index_search(ivr_pqfs_index *idx, const uint8_t *U /*DEV [nq][M][16]*/, const float *scale /*DEV [nq]*/,
                          const float *bias /*DEV [nq]*/, int nq, int k, float *D /*DEV [nq][k]*/, int64_t *I /*DEV [nq][k]*/,
                          ivr_stream stream);

/* ---- graph index (in the place of faiss IndexHNSWFlat) ------------------------------------------------------
 * Stands in for faiss.IndexHNSWFlat(dimension, 32), the IndexHNSW type of _create_index (core.py:1213-1214).  It is NOT a port of
 * faiss's HNSW: one layer of fixed out-degree (2 M, HNSW's level-0 width), built in bulk from exact kNN lists, entered through
 * caller-chosen entry rows, inner product only ("graph index"; the definitions are the numpy functions of
 * ivr_amd/graph.py).  Row numbers are int32 positions in [0, ntotal), -1 = none.  Every order is (score descending, row ascending):
 * the (ordered score, ~row) key of ivr_index_search.  A score is accumulated in the summation order of ivr_index_search and so
 * carries its bits for the same pair.
 * The object keeps a ROW-MAJOR float32 copy of the rows, each padded with zeros to a multiple of 16 floats, so that four lanes read
 * 64 contiguous bytes of a neighbour (the tiled layout of ivr_index spaces the quads of a row 256 bytes apart), and the int32
 * neighbour table [ntotal][degree].  One stream at a time per handle. */
typedef struct ivr_graph ivr_graph;
#define IVR_GRAPH_MAX_EF 256        /* longest candidate list of a search (ef), and so the largest k */
#define IVR_GRAPH_MAX_CAND 64       /* most candidates per row ivr_graph_prune takes (efConstruction) */
#define IVR_GRAPH_MAX_DEGREE 64     /* largest out-degree, and most entry rows per query */
int ivr_graph_max_ef(void);         /* the two limits as the library was built (core.py:1213-1214) */
int ivr_graph_max_cand(void);
/* core.py:1213-1214.  1 <= d <= 8192, 1 <= degree <= IVR_GRAPH_MAX_DEGREE */
int ivr_graph_create(ivr_ctx *ctx, int d, int degree, ivr_graph **out);
int ivr_graph_destroy(ivr_graph *g);                        /* core.py:1213-1214 */
int ivr_graph_reset(ivr_graph *g);                          /* core.py:1213-1214: ntotal = 0, no neighbours */
int64_t ivr_graph_ntotal(ivr_graph *g);                     /* core.py:1213-1214 */
/* core.py:1213-1214.  Replace the stored rows by the n given ones (n < 2^31; n == 0 empties the object) and forget the neighbour
 * table.  A call that grows the allocation synchronises the device. */
int ivr_graph_set_rows(ivr_graph *g, const float *rows /*DEV [n,d] row-major*/, int64_t n, ivr_stream stream);
/* core.py:1213-1214.  HNSW's neighbour-selection heuristic (faiss shrink_neighbor_list with distance -ip) on the stored rows, one
 * workgroup per base row r: walk cand[r] in order, keep c iff <c, g> <= <r, c> for every g kept so far, stop at M kept; the rest of
 * nbr[r] is -1 with score 0.  nbr_score[r][i] = <r, nbr[r][i]>.  Entries of cand outside [0, ntotal) are skipped.  The C x C Gram
 * matrix of the candidates and the base scores run on the float32 MFMA.  1 <= C <= IVR_GRAPH_MAX_CAND, 1 <= M <= 64.  Enqueue-only. */
int ivr_graph_prune(ivr_graph *g, const int32_t *cand /*DEV [n][C]*/, int C, int M, int32_t *nbr /*DEV [n][M]*/,
                    float *nbr_score /*DEV [n][M]*/, ivr_stream stream);
/* core.py:1213-1214.  Install the neighbour table (copied); n must equal ntotal.  Entries outside [0, ntotal) are never
 * dereferenced by a search: it skips them. */
int ivr_graph_set_neighbors(ivr_graph *g, const int32_t *graph /*DEV [n][degree]*/, int64_t n, ivr_stream stream);
/* core.py:1213-1214.  Best-first walk of the graph, one workgroup per query (graph_search_ref of ivr_amd/graph.py):
 *   L := the distinct valid rows of entries[q] with their scores, in order, cut to ef
 *   at most max_expansions times: cur := the first row of L not yet expanded (none: stop); new := the distinct valid neighbours of
 *   cur that are not in L, scored; L := the first ef of sort(L + new)
 *   D / I := the first k of L; unused slots (-FLT_MAX, -1) as ivr_index_search leaves them; n_expanded[q] := rows expanded.
 * 1 <= k <= ef <= IVR_GRAPH_MAX_EF, 1 <= ne <= IVR_GRAPH_MAX_DEGREE, 1 <= nq <= 2^22; max_expansions is clamped to [1, max(ntotal, 1)], so
 * every loop of the kernel is bounded by it and by the degree.  normalize_q: the queries are L2-normalised first (into scratch).
 * IVR_ERR_STATE while rows are stored without a neighbour table; an empty object returns unused slots only.  Scratch: nq d floats
 * when normalize_q, else nothing.  Enqueue-only once that scratch has grown. */
int ivr_graph_search(ivr_graph *g, const float *q /*DEV [nq,d]*/, int nq, int k, int ef, const int32_t *entries /*DEV [nq][ne]*/, int ne,
                     int max_expansions, int normalize_q, float *D /*DEV [nq,k]*/, int64_t *I /*DEV [nq,k]*/,
                     int32_t *n_expanded /*DEV [nq] or NULL*/, ivr_stream stream);

/* Merge per-shard candidate lists (the reference's concat + sort of peer results, system.py:1744-1746):
 * D_parts/I_parts DEV [parts, nq, k] with global ids, parts ordered by ascending id range. */
int ivr_topk_merge(ivr_ctx *ctx, const float *D_parts /*DEV*/, const int64_t *I_parts /*DEV*/, int parts,
                   int nq, int k, float *D /*DEV*/, int64_t *I /*DEV*/, ivr_stream stream);

/* The same merge straight from the buffer of the ONE all-gather of the sharded search: a candidate travels as three int32 words
 * (score bits, id low, id high), so the exchange is pack (one launch) -> all_gather_into_tensor -> merge (one launch).
 * packed: DEV int32 [nq,k,3]; packed_parts: DEV int32 [parts,nq,k,3], parts ordered by ascending id range. */
int ivr_topk_pack(ivr_ctx *ctx, const float *D /*DEV*/, const int64_t *I /*DEV*/, int nq, int k, int32_t *packed /*DEV*/,
                  ivr_stream stream);
int ivr_topk_merge_packed(ivr_ctx *ctx, const int32_t *packed_parts /*DEV*/, int parts, int nq, int k, float *D /*DEV*/,
                          int64_t *I /*DEV*/, ivr_stream stream);

/* ---- D1: near-duplicate frame filter ------------------------------------------------------------
 * Replaces the cosine_similarity(...) >= SIM_THRESHOLD loop at video_frame_filter.py:63-70.
 * emb: DEV float32 [n,d] in frame order.  keep[t] = 1 iff cos(emb[t], last kept) < threshold.
 * state: DEV float32 [d+1]: state[0] = 1 if a previous kept embedding is stored in state[1..d];
 * updated in place so consecutive batches of one video continue the same sequence.
 */
int ivr_dedup_keep_mask(ivr_ctx *ctx, const float *emb /*DEV*/, int n, int d, float threshold,
                        float *state /*DEV*/, uint8_t *keep /*DEV*/, ivr_stream stream);

/* In-scene similarity filter of the keyframe pipeline, filter_similar_frames_in_scene at filter.py:178-222, as ONE launch per
 * scene: emb DEV float32 [n,d] = the scene's frames in order; keep[0] = 1; keep[i] = 1 iff i is at least min_distance after the
 * last kept frame and cos(emb[i], emb[last kept]) < threshold (the caller appends the scene's last frame, filter.py:218-220). */
int ivr_scene_keep_mask(ivr_ctx *ctx, const float *emb /*DEV*/, int n, int d, float threshold, int min_distance,
                        uint8_t *keep /*DEV*/, ivr_stream stream);

/* Window variant, filter_similar_frames_advanced at filter.py:224-258 (selected by use_advanced_similarity_filtering, filter.py:292-295):
 * keep[0] = 1; keep[i] = 1 iff no KEPT frame j in [i - min(window, n), i) has cos(emb[i], emb[j]) >= threshold.  Two launches: the
 * banded cosines in parallel, then the decision chain over n x window floats. */
int ivr_scene_keep_mask_window(ivr_ctx *ctx, const float *emb /*DEV*/, int n, int d, float threshold, int window,
                               uint8_t *keep /*DEV*/, ivr_stream stream);

/* cos(a[i], b[i]) for i < n (DEV float32 [n,d] each), sklearn cosine_similarity conventions.  Replaces the per-pair
 * cosine_similarity([x],[y])[0][0] calls of the keyframe filter (filter.py:147, filter.py:208). */
int ivr_rowwise_cosine(ivr_ctx *ctx, const float *a /*DEV*/, const float *b /*DEV*/, int n, int d, float *out /*DEV*/,
                       ivr_stream stream);

/* ---- look-back filters of the research keyframe extractor ---------------------------------------------
 * Both walk the rows of every segment [seg_off[s], seg_off[s+1]) (seg_off: DEV int64 [nseg+1], ascending, clipped to [0, n); NULL
 * with nseg = 0: one segment of all rows) in row order and hold a window of the last `window` KEPT rows of that segment,
 * 1 <= window <= IVR_KEEPWIN_MAX_WINDOW; a kept row is appended, and the oldest leaves once the window holds more than `window`.
 * keep: DEV uint8 [n]; rows outside every segment get 0.  Segments run in parallel, the rows of one segment are a serial chain.
 *
 * ivr_hash_keep_mask: the perceptual-duplicate filter of filter_research_update.py:157-162 and :289-298.  hashes: DEV uint8 [n,8];
 * row i is kept iff no hash h in the window has popcount(hashes[i] xor h) <= threshold.
 *
 * ivr_kept_window_mask: the final temporal filter of filter_research_update.py:316-338.  emb: DEV float32 [n,d]; row i is kept iff
 * no row j in the window has cos(emb[i], emb[j]) >= threshold, the cosine with the arithmetic of ivr_rowwise_cosine.  Unlike
 * ivr_scene_keep_mask_window the window counts kept rows, not predecessors, so it reaches arbitrarily far back.  Scratch (the
 * squared norms, n floats) lives in the context, per stream. */
#define IVR_KEEPWIN_MAX_WINDOW 64
int ivr_hash_keep_mask(ivr_ctx *ctx, const uint8_t *hashes /*DEV*/, int64_t n, const int64_t *seg_off /*DEV or NULL*/, int nseg,
                       int threshold, int window, uint8_t *keep /*DEV*/, ivr_stream stream);
int ivr_kept_window_mask(ivr_ctx *ctx, const float *emb /*DEV*/, int64_t n, int d, const int64_t *seg_off /*DEV or NULL*/, int nseg,
                         float threshold, int window, uint8_t *keep /*DEV*/, ivr_stream stream);

/* ---- frame quality gating of the keyframe filter ---------------------------------------------------
 * Replaces calculate_blur_score / calculate_edge_density at filter.py:63-92 (cv2.Laplacian(gray, CV_64F).var() and the share of
 * cv2.Canny(gray, low, high) edge pixels) for a batch of decoded frames.  frames: DEV uint8 [n,h,w,3] (bgr = 1: cv2.imread
 * order, 0: RGB).  lap_sums: DEV int64 [n,2] = (sum, sum of squares) of the integer Laplacian response over the frame - the
 * variance is (s2 - s1*s1/N) / N with N = h*w, finished in float64 by the caller; edge_count: DEV int64 [n] = number of Canny
 * edge pixels (edge density = 100 * count / N).  w <= 16384.  Scratch (two bit planes = 2 bits per pixel, rows padded to 64 pixels, + 16 B per
 * 64 x 32 tile) lives in the context, per stream. */
int64_t ivr_frame_quality_scratch_bytes(int n, int h, int w);
int ivr_frame_quality(ivr_ctx *ctx, const uint8_t *frames /*DEV*/, int n, int h, int w, int bgr, int canny_low, int canny_high,
                      int64_t *lap_sums /*DEV*/, int64_t *edge_count /*DEV*/, ivr_stream stream);

/* ---- diversified search: maximal marginal relevance and near-duplicate suppression over candidate lists ----
 * Which k of the kc candidates of a query answer it without showing one picture k times?  Adjacent keyframes of a shot, the same scene
 * in two videos and a recurring shot lie within a hair of each other in cosine and fill the head of a relevance-ranked list.  Vector
 * stores answer with MMR (LangChain's max_marginal_relevance_search, Qdrant, Elasticsearch, OpenSearch) or by dropping a hit that is
 * nearly the same as a better one.  cand is positional like ivr_index_rescore, on plain and id-mapped indexes alike; an entry outside
 * [0, ntotal), -1 included, is absent; a row named twice is two candidates.
 *   relevance   R[j] = the float32 score ivr_index_rescore reports for (query q, row cand[q][j]), so the bits of ivr_index_search
 *   pair score  P[i, j] = the float32 score ivr_index_rescore reports for (query = the stored float32 row cand[q][i], row cand[q][j]):
 *               the chosen row is the query operand.  Both enter the arithmetic as reported, -0.0 as +0.0
 *   order       candidates rank by (value descending, -0.0 equal to +0.0; row ascending; position in cand ascending)
 *   selection   greedy, t = 0 .. k - 1; m[j] = the greatest P[s, j] over the candidates s chosen so far, by float compare
 *   IVR_DIVERSE_MMR       param = lambda in [0, 1], mu = 1.0f - lambda.  The first choice is the best candidate by R, what
 *                         ivr_index_search returns first whatever lambda is; from the second on the value of a candidate not yet chosen
 *                         is (lambda * R[j]) - (mu * m[j]): two float32 products and one float32 subtraction, each rounded, no fused
 *                         multiply-add.  lambda = 1 is the order of ivr_index_rescore
 *   IVR_DIVERSE_SUPPRESS  param = threshold.  The value is R[j]; a candidate with m[j] >= threshold is out for good, and the selection
 *                         ends early when nothing is left.  A threshold above every P is the order of ivr_index_rescore, one below every
 *                         P returns one result
 * D DEV [nq][k]: R of each chosen candidate, in the order chosen; I DEV [nq][k]: its row, or its stored id on an id-mapped index; M DEV
 * [nq][k] or NULL: m of the chosen candidate at the moment it was chosen (how redundant is this hit?), -FLT_MAX in slot 0.  Unused slots
 * hold -FLT_MAX / -1 / -FLT_MAX.  1 <= k <= kc <= IVR_MAX_K, nq >= 1, nq kc < 2^31, mode one of the two constants, param not NaN and
 * within [0, 1] for IVR_DIVERSE_MMR; anything else is IVR_ERR_INVALID, checked before any device call.  An empty index gives unused
 * slots only.
 *
 * Two launches on `stream`: the relevance scores (the first launch of ivr_index_rescore), then one workgroup per query that keeps R, m,
 * the rows and a state byte of its candidates in LDS (13 bytes each) and runs the k steps: pick the best candidate, then score the
 * chosen row, read from the storage tiles as it lies, against the candidates still in play.  P is scored lazily, k kc d multiply-adds
 * per query instead of kc kc d; the steps of a query are sequential on one compute unit, so a single query at large k is the worst
 * case.  Scratch: 4 bytes per (query, candidate), grow-only.  Enqueue-only once the scratch has grown (a call that grows it allocates);
 * not graph-capturable then.  The same bits on every run and stream. */
#define IVR_DIVERSE_MMR      0
#define IVR_DIVERSE_SUPPRESS 1
int ivr_index_diversify(ivr_index *idx, const float *q /*DEV [nq,d]*/, int nq, const int64_t *cand /*DEV [nq][kc]*/, int kc, int k,
                        int mode, float param, int normalize_q, float *D /*DEV [nq][k]*/, int64_t *I /*DEV [nq][k]*/,
                        float *M /*DEV [nq][k] or NULL*/, ivr_stream stream);

/* ---- fused search: one ranking of the stored rows from a set of query vectors per query ---------------
 * Several expansions of one text, a text and an example image, "like these frames but not like that one", "all of these concepts in
 * one frame": every other search ranks the rows against ONE vector per query, and joining m result lists on the host invents a score
 * for a row that misses a list and, for a minimum, looks in the wrong place altogether.  Here every stored row is scored against every
 * member and folded in registers; the result is exact over all rows.  This is the library's own definition (vector stores have
 * relatives: multi-vector queries, Qdrant's recommend API with its best_score strategy), not parity with any of them.
 * q: DEV float32 [nq][slots][d], slots one of 1, 2, 4, 8, 16 (IVR_FUSE_MAX_MEMBERS): the member vectors of fused query f are rows
 * f * slots .. f * slots + slots - 1.  w: DEV float32 [nq][slots], every entry finite.  role: DEV int8 [nq][slots]: 1 a positive member,
 * -1 a negative one, 0 an absent slot (its vector and weight are not used; pass zeros).  Every set needs a positive member.
 *   member score  S[j, r] = the float32 inner product ivr_index_search reports for (member j, stored row r), to the bit (-0.0 as +0.0)
 *   T[j]          = w[j] * S[j, r]: one float32 product, rounded on its own, never fused with what follows
 *   P             the fold of T over the positive members.  IVR_FUSE_MAX: the maximum (expansion, OR).  IVR_FUSE_MIN: the minimum (AND).
 *                 IVR_FUSE_SUM: the balanced pairwise tree over the `slots` slots of the set, ((T0 + T1) + (T2 + T3)) + ..., in which a
 *                 slot that is absent or negative contributes +0.0f: NOT an ascending sum, and the same set staged at another `slots` or
 *                 in another slot order may differ in the last bit
 *   Nn            the maximum of T over the negative members
 *   F             a set without negative members: P.  IVR_FUSE_MARGIN: P - Nn, one float32 subtraction.  IVR_FUSE_VETO: P when P > Nn,
 *                 else -(Nn * Nn), one product and one negation: a row that resembles a negative example at least as much as any
 *                 positive one sinks, the further the more it resembles it
 *   order         rows rank by (F descending, -0.0 equal to +0.0; row ascending), the result key of every top-k of the library
 * Results are labelled with the row, or with its stored id on an id-mapped index; scores are written as every search writes them
 * (-0.0 as +0.0).  normalize_q scales every member vector to unit length first, as everywhere else.
 * ivr_index_search_fused: D / I DEV [nq][k], the k best rows of each fused query; unused slots (-FLT_MAX, -1).  1 <= k <= IVR_MAX_K.
 * ivr_index_range_search_fused: every row with F >= threshold, in the form of ivr_index_range_search_sequences: lims DEV int64
 * [nq + 1], lims[0] = 0, the rows of fused query f at [lims[f], lims[f + 1]) in ascending row order; entries at positions >= cap are
 * counted but not written.  A NaN threshold is IVR_ERR_INVALID (+-inf are allowed).
 * IVR_ERR_INVALID with a message in ivr_last_error, before anything is launched: slots not one of 1, 2, 4, 8, 16; nq < 1; nq * slots
 * >= 2^31; an unknown fold or combine; k outside [1, IVR_MAX_K]; a role outside {1, -1, 0}; a weight that is not finite; a set without
 * a positive member; ntotal >= 2^31.  An empty index gives unused slots / lims of zeros.
 *
 * Launches per chunk of fused queries, all on `stream`: the score pass of the clip search, whose epilogue writes no score: a set is an
 * aligned group of `slots` columns of the 16-column query tile, each lane forms T for its column, the positive and the negative
 * accumulator are folded across the set with log2(slots) cross-lane exchanges, and one lane per set writes the 64-bit keys of its four
 * rows into the fused query's stretch of the key scratch; then the top-k selection over the stretch, or the count / prefix / write
 * passes of the range form with the running total carried on the device.  Scratch on the index, grow-only: 8 bytes per (fused query of
 * a chunk, stored row rounded up to 16) with at most IVR_SEQ_CHUNK_SLOTS slots per chunk, in whole query tiles (one tile = 16 / slots
 * fused queries at least, 4,096 columns at most).  The role and weight tables are checked on the host: the call copies them back (5
 * bytes per slot) and waits for `stream` once, before its first launch; after that it only enqueues (a call that grows the scratch
 * allocates).  Not graph-capturable.  The same bits on every run and stream. */
#define IVR_FUSE_MAX_MEMBERS 16
#define IVR_FUSE_MAX    0
#define IVR_FUSE_MIN    1
#define IVR_FUSE_SUM    2
#define IVR_FUSE_MARGIN 0
#define IVR_FUSE_VETO   1
int ivr_index_search_fused(ivr_index *idx, const float *q /*DEV [nq*slots,d]*/, int nq, int slots, const float *w /*DEV [nq*slots]*/,
                           const int8_t *role /*DEV [nq*slots]: 1, -1, 0*/, int fold, int combine, int k, int normalize_q,
                           float *D /*DEV [nq,k]*/, int64_t *I /*DEV [nq,k]*/, ivr_stream stream);
int ivr_index_range_search_fused(ivr_index *idx, const float *q /*DEV [nq*slots,d]*/, int nq, int slots, const float *w /*DEV [nq*slots]*/,
                                 const int8_t *role /*DEV [nq*slots]: 1, -1, 0*/, int fold, int combine, float threshold, int normalize_q,
                                 int64_t *lims /*DEV [nq+1]*/, float *D /*DEV [cap]*/, int64_t *I /*DEV [cap]*/, int64_t cap,
                                 ivr_stream stream);

#ifdef __cplusplus
}
#endif
#endif /* IVR_API_H */
