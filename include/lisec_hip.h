/*
 * lisec_hip.h -- C ABI of the MI355X (gfx950) hot path of Lisec.
 *
 * The reference (bot15498/Lisec) has no FFI: its hot path is Python calling
 * TensorFlow/Keras.  Every entry point below replaces one group of reference
 * statements; the citation is file:line in the reference tree.
 *
 * Conventions
 *   - plain C types only; every pointer marked "dev" is a device (HBM) pointer the
 *     CALLER owns; nothing here allocates or frees device memory;
 *   - every function takes the HIP stream to enqueue on (void* == hipStream_t) and
 *     returns immediately after enqueueing; no host synchronisation inside;
 *   - return value: 0 ok, < 0 error (LISEC_E*), message via lisec_last_error()
 *     (thread local);
 *   - scratch memory comes from the caller: *_workspace_bytes() says how much;
 *   - tensors are channels-last fp32, exactly the Keras layouts of the reference:
 *       activations (D,H,W,C) / (H,W,C); Dense kernel (in,out);
 *       Conv3D kernel (kd,kh,kw,in,out); Conv2D (kh,kw,in,out);
 *       Conv2DTranspose (kh,kw,out,in).
 */
#ifndef LISEC_HIP_H
#define LISEC_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LISEC_OK 0
#define LISEC_EINVAL (-1)   /* bad argument / shape the kernels do not support */
#define LISEC_ENOSPC (-2)   /* workspace or output capacity too small           */
#define LISEC_EHIP (-3)     /* a HIP runtime call failed                        */

typedef void* lisec_stream_t; /* hipStream_t */

const char* lisec_last_error(void);
/* ABI version, bumped on any signature change. */
int lisec_abi_version(void);
/* Fills name (<= cap bytes) with the device's gcnArchName; returns CU count or < 0. */
int lisec_device_info(char* name, int cap);

/* ------------------------------------------------------------------------------------------
 * 1. Voxeliser  -- replaces get_voxel + VFE_preprocessing + sparse.to_dense
 *    (model_training.py:103-152, :279; Predict.py:21-30).
 * ------------------------------------------------------------------------------------------ */
typedef struct {
    double xSize, ySize, zSize;            /* Constants.voxelx/y/z                      */
    int maxVoxelX, maxVoxelY, maxVoxelZ;   /* Constants.nx//2, ny//2, nz                */
    int sampleSize;                        /* Constants.maxPoints (T), <= 64            */
} lisec_voxel_cfg;

/* Header written by lisec_voxelize at the start of `info` (device int32[8]). */
enum { LISEC_VI_NVOX = 0, LISEC_VI_NROWS = 1, LISEC_VI_NVALID = 2, LISEC_VI_MAXCOUNT = 3,
       LISEC_VI_OVERFLOW = 4 };

/* Optional per-sweep side output of lisec_voxelize, input of lisec_vfe_forward: int64[LISEC_ROW_STATS_WORDS].
 *   words [0, LISEC_ROW_STATS_MOMENT_WORDS): the first and second moments of the feature rows -- sum of x_k (6) and
 *     of x_j*x_k (21, j <= k) over all kept rows, as order-independent two-limb fixed-point sums in
 *     LISEC_ROW_STATS_REPLICAS replicas ([replica][27][2]).  The first Dense of the VFE stack has no bias and no
 *     activation in front of its BatchNormalization (model_training.py:171-173,184), so the batch statistics of that
 *     layer are a closed form of these moments and of the kernel: the VFE needs no pass over the rows for them.
 *   the remaining words: scratch of lisec_vfe_forward, zeroed by lisec_voxelize and left zeroed by every forward. */
#define LISEC_ROW_STATS_REPLICAS 16
#define LISEC_ROW_STATS_MOMENT_WORDS (LISEC_ROW_STATS_REPLICAS * 27 * 2)
#define LISEC_ROW_STATS_WORDS (LISEC_ROW_STATS_MOMENT_WORDS + 4 * 64 * 2)

size_t lisec_voxelize_workspace_bytes(const lisec_voxel_cfg* cfg, int n_points);

/*
 * points      dev  n_points rows of `point_stride` elements, first three = x, y, z
 *                  (dtype: 0 = float32, 1 = float64; the reference feeds float64,
 *                  model_training.py:93-96)
 * cap_voxels       capacity of the per-voxel outputs (V <= min(n_points, cells))
 * info        dev  int32[8]   see LISEC_VI_*
 * cell_voxel  dev  int32[NZ*NX*NY]  voxel ordinal of every grid cell, -1 if empty
 * coords      dev  int32[cap_voxels*3]  (z, x, y) as model_training.py:148, sorted by cell
 * counts      dev  int32[cap_voxels]    raw in-range point count
 * npts        dev  int32[cap_voxels]    min(count, sampleSize)
 * row_start   dev  int32[cap_voxels+1]  exclusive prefix of npts
 * rows        dev  float32[n_points*6]  compact feature rows [x,y,z,x-cx,y-cy,z-cz]
 *                  (model_training.py:135-140), voxel v owns rows row_start[v]..+npts[v];
 *                  ascending original point index, first sampleSize kept
 * row_point   dev  int32[n_points] or NULL: original point index of every row
 * row_stats   dev  int64[LISEC_ROW_STATS_WORDS] or NULL: see above
 */
int lisec_voxelize(const lisec_voxel_cfg* cfg, const void* points, int dtype, int n_points,
                   int point_stride, void* workspace, size_t workspace_bytes, int cap_voxels,
                   int32_t* info, int32_t* cell_voxel, int32_t* coords, int32_t* counts,
                   int32_t* npts, int32_t* row_start, float* rows, int32_t* row_point,
                   int64_t* row_stats, lisec_stream_t stream);

/* 1b. The reference's random subsample of a crowded voxel (np.random.choice(bucket, size=35, replace=False),
 *     model_training.py:131-132; VoxelNet section 2.1.1), seeded.  lisec_voxelize_draw is lisec_voxelize with one rule
 *     changed, for voxels with count > sampleSize only.  Random numbers are those of section 5c: Philox4x32-10, key = seed
 *     (low word, high word), counter = (stream, item, epoch, index); this draw is stream 4 and `index` is the point's row
 *     index in `points`.  Point i of such a voxel has the 64-bit key (Philox(4, item, epoch, i)[0] << 32) | i; the
 *     sampleSize points with the smallest keys are kept (the low word breaks equal Philox words, so the rule is total) and
 *     emitted in ASCENDING POINT INDEX, as lisec_voxelize emits its rows.  Centroid, feature rows, row_point and row_stats
 *     follow from the kept points exactly as there.  Voxels with count <= sampleSize, and coords, counts, npts,
 *     row_start, cell_voxel and info, are those of lisec_voxelize bit for bit.  The key depends on the point index alone
 *     -- not on the order the points reach their voxel, not on rows behind the sweep -- so the result is deterministic
 *     and the same for a sweep padded to a fixed capacity with rows outside the grid as for the bare sweep.
 *   draw  dev  uint32[4] = seed low word, seed high word, item, epoch, READ BY THE KERNEL when it runs: a recorded step plan
 *     (section 5b) replays with whatever the words hold then.  lisec_voxel_draw_set writes them with a one-thread kernel
 *     on `stream` (scalar arguments, no host synchronisation; recorded like any launch when the thread records a plan).
 *     draw == NULL: LISEC_EINVAL, nothing enqueued.  The workspace is that of lisec_voxelize. */
int lisec_voxelize_draw(const lisec_voxel_cfg* cfg, const void* points, int dtype, int n_points,
                        int point_stride, void* workspace, size_t workspace_bytes, int cap_voxels,
                        int32_t* info, int32_t* cell_voxel, int32_t* coords, int32_t* counts,
                        int32_t* npts, int32_t* row_start, float* rows, int32_t* row_point,
                        int64_t* row_stats, const uint32_t* draw, lisec_stream_t stream);
int lisec_voxel_draw_set(uint32_t* draw, unsigned long long seed, unsigned int item, unsigned int epoch,
                         lisec_stream_t stream);

/* Expands compact rows into the zero padded (V, T, 6) block layout the reference's
 * SparseTensor / dense tensor uses (model_training.py:141-152).  padded: float32[V*T*6]. */
int lisec_voxel_rows_to_padded(const int32_t* info, const int32_t* npts, const int32_t* row_start,
                               const float* rows, int sampleSize, int cap_voxels, float* padded,
                               lisec_stream_t stream);

/* Lidar ingest (rotate_points + translation of combine_lidar_data, model_training.py:65-98):
 * out[i] = R * raw[i, :3] + t in float64; raw: device float32 rows of raw_stride (5 for Lyft .bin files);
 * rotation9: HOST row-major 3x3 rotation matrix of the sensor quaternion, translation3: HOST;
 * out: device float64 (n,3) -- typically a slice of the concatenated cloud handed to lisec_voxelize. */
int lisec_lidar_transform(const float* raw, int n_points, int raw_stride, const double* rotation9,
                          const double* translation3, double* out, lisec_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * 2. VFE stack (sparse-exact) -- replaces addVFELayer(6,32) + addVFELayer(32,64) + addFCN(64,64)
 *    + MaxPoolingVFELayer(combine=True) (model_training.py:155-186, :231-235, layers :32-61) on the
 *    dense (D,H,W,T,6) input; output is the dense (D,H,W,64) grid the first Conv3D reads (:236).
 * ------------------------------------------------------------------------------------------ */
typedef struct {
    const float* kernel[3];   /* Dense(use_bias=False) kernels (6,16) (32,32) (64,64)  (:184)          */
    const float* gamma[3];    /* BatchNormalization() variables, 16 / 32 / 64 channels (:171)          */
    const float* beta[3];
    float* moving_mean[3];    /* updated in place by a training forward (momentum 0.99)                */
    float* moving_var[3];
} lisec_vfe_params;

/* Size (floats) of the `saved` buffer a forward fills and the backward reads: BN batch statistics
 * and the per-voxel pre-BN max/min of each layer. */
size_t lisec_vfe_saved_floats(int cap_voxels);
/* The same plus the per-row extras a training forward can leave for the tiled (MFMA) backward: the slot of the first
 * row holding each per-voxel maximum / minimum, and the layer-2 pre-BN value of every class row.  n_points = the row
 * capacity (rows <= n_points).  Pass the same n_points to lisec_vfe_forward and LISEC_VFE_BWD_TILED to the backward. */
size_t lisec_vfe_saved_floats_rows(int cap_voxels, int n_points);
/* Offsets (in floats) inside `saved` of the compact per-voxel outputs written by every forward:
 *   VOUT  float[(cap+1)*64]  grid value of voxel v; row V = the constant every empty cell holds
 *   DELTA float[(cap+1)*64]  VOUT[v] - VOUT[V] */
enum { LISEC_VFE_SAVED_VOUT = 0, LISEC_VFE_SAVED_DELTA = 1 };
size_t lisec_vfe_saved_field_offset(int cap_voxels, int field);
size_t lisec_vfe_workspace_bytes(void);

/*
 * info/cell_voxel/npts/row_start/rows: outputs of lisec_voxelize (device).
 * ncells = NZ*NX*NY, T = sampleSize.  training != 0: batch statistics (Keras fit), moving stats
 * updated; training == 0: moving statistics (Keras predict, Predict.py:38).
 * row_stats: the voxeliser's side output (NULL: the moments are summed here, one more launch).
 * n_points: 0, or the row capacity `saved` was sized for with lisec_vfe_saved_floats_rows (training only: the
 *           per-row extras are then written).
 * grid  dev float32[ncells*64]: (D,H,W,64), every cell written (empty cells hold relu(BN3(.)) != 0); NULL = only
 *       the compact per-voxel outputs (VOUT / DELTA in `saved`), the input of lisec_conv_field_forward.
 */
int lisec_vfe_forward(const lisec_vfe_params* p, const int32_t* info, const int32_t* cell_voxel,
                      const int32_t* npts, const int32_t* row_start, const float* rows, int64_t* row_stats,
                      int n_points, int ncells, int T, int cap_voxels, int training, float* saved, void* workspace,
                      size_t workspace_bytes, float* grid, lisec_stream_t stream);

/* Re-materialises the dense grid from the `saved` buffer of the last lisec_vfe_forward (the HBM-bound
 * writer on its own: lets a caller recycle the 164 MB grid buffer, and lets bench.py time the writer). */
int lisec_vfe_grid_from_saved(const int32_t* info, const int32_t* cell_voxel, int ncells, int cap_voxels,
                              const float* saved, float* grid, lisec_stream_t stream);

/* Gradients of the VFE variables (what fit() derives for the layers of :231-235), training-mode BN.
 * dgrid: float32[ncells*64], gradient wrt the grid written by lisec_vfe_forward(training=1);
 * saved: the buffer that forward filled.  Outputs are written (not accumulated). */
typedef struct {
    float* kernel[3];   /* (6,16) (32,32) (64,64) */
    float* gamma[3];
    float* beta[3];
} lisec_vfe_grads;
#define LISEC_VFE_BWD_TILED 1   /* flags: `saved` carries the per-row extras of lisec_vfe_forward(n_points > 0): layers 3
                                   and 2 run on 32-row tiles on the matrix cores instead of row by row per voxel */
size_t lisec_vfe_backward_workspace_bytes(int cap_voxels, int n_points);
/* Pass EITHER dgrid (dense gradient of the grid) OR the compact form the sparse backward of the first middle
 * layer produces: dout_rows float[(cap_voxels+1)*64] with rows [0,V) = gradient at the occupied cells (row V is
 * written here) and g_all float[64] = sum of the grid gradient over ALL cells. */
int lisec_vfe_backward(const lisec_vfe_params* p, const int32_t* info, const int32_t* cell_voxel,
                       const int32_t* npts, const int32_t* row_start, const float* rows, int n_points,
                       int ncells, int T, int cap_voxels, const float* saved, const float* dgrid,
                       float* dout_rows, const float* g_all, const lisec_vfe_grads* grads, int flags, void* workspace,
                       size_t workspace_bytes, lisec_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * 3. Dense contractions on the fp32 matrix cores (implicit GEMM, no im2col buffer).
 *    One geometry descriptor covers Conv3D (model_training.py:192-193), Conv2D (:202-203),
 *    Conv2DTranspose (:246,:249,:252), Dense on the last axis (:184,:195), the 1x1 heads (:254-255)
 *    and the data gradients of all of them.
 * ------------------------------------------------------------------------------------------ */
typedef struct {
    int mode;           /* 0: conv,  src = o*stride - pad + k   (ZeroPaddingND + 'valid', cross-correlation)
                           1: transposed conv, src = (o + pad - k)/stride when divisible
                              (Conv2DTranspose forward; data gradient of a mode-0 conv)                */
    int Di, Hi, Wi;     /* spatial dims of the tensor gathered from (2D: Di = 1)                       */
    int Do, Ho, Wo;     /* spatial dims of the tensor written                                          */
    int KD, KH, KW;     /* kernel taps                                                                 */
    int sd, sh, sw;     /* strides: 1, 2 or 4                                                          */
    int pd, ph, pw;     /* ZeroPadding (mode 0) / padding of the conv this is the transpose of (mode 1) */
    int Cin, in_stride;   /* channels contracted over; floats between positions of `in` (>= Cin)       */
    int Cout, out_stride; /* channels produced; floats between positions of `out` (concat: 768)        */
    int ps, ps_channels;  /* "pixel-shuffle" store for a Conv2DTranspose whose kernel == stride (:249,:252),
                             run as a 1x1 conv with Cout = ps*ps*ps_channels: result column tap*ps_channels+n of
                             input position (h,w) is stored at position (h*ps+kh, w*ps+kw), channel n
                             (tap = kh*ps+kw) of a (Ho*ps, Wo*ps) map; bias is indexed by n.  0 = off.       */
} lisec_conv_geom;

#define LISEC_CONV_IN_RELU 1     /* apply ReLU to the gathered input (after the optional affine)        */
#define LISEC_CONV_OUT_RELU 2    /* apply ReLU before the store (Dense(..., 'relu'), :195)              */
#define LISEC_CONV_ACCUMULATE 4  /* out += result (gradient fan-in)                                     */
#define LISEC_CONV_TAG_ROOFLINE 32 /* measurement aid: one un-sliced launch under the symbol k_igemm<0,false,1>
                                     (lisec_conv_forward_winograd: k_wino<false,0,1>), so a rocprofv3 --stats row
                                     shows this layer alone (bench.py roofline)                                    */
#define LISEC_CONV_DY_RELU 8     /* wgrad only: ReLU on the (optionally affine-transformed) dy operand     */
#define LISEC_CONV_SMALL_TILE 16 /* lisec_conv_forward*: a small K-sliced layer may run as 64-row tiles, two workgroups per CU
                                    (k_igemm_small; lisec_tuning.small_tile).  Same output and statistics, bit for bit (with a
                                    sink the call needs the workspace).  Ignored where the kernel does not serve the call:
                                    see lisec_conv_plan.tile_rows                                                      */

/* Packed weight layout the kernels read: [tap][K/4][N][4] fp32, K and N zero padded to 64.
 * src element (tap, k, n) is read at src[tap*tap_stride + k*k_stride + n*n_stride], so any Keras
 * kernel layout (and its transpose for the data gradient) packs without a host-side copy. */
size_t lisec_conv_packed_floats(int ntaps, int K, int N);
int lisec_conv_pack_weights(const float* src, int ntaps, int K, int N, long long tap_stride,
                            long long k_stride, long long n_stride, float* dst, lisec_stream_t stream);

/* The same repack for many kernels in one launch (the whole network after an optimizer step).  The table
 * lives in DEVICE memory; start = running sum of ntaps*Kp*Np (Kp, Np = K, N rounded up to 64); total = the
 * sum over all entries. */
typedef struct {
    const float* src;
    float* dst;
    long long tap_stride, k_stride, n_stride, start;
    int ntaps, K, N, Kp, Np, pad_;
} lisec_pack_desc;
int lisec_conv_pack_weights_batched(const lisec_pack_desc* device_table, int n, long long total,
                                    lisec_stream_t stream);

/* Number of 128-row tiles = leading dimension of `stats_partials`. */
int lisec_conv_num_mblocks(const lisec_conv_geom* g);

/*
 * out[m, n] = sum_tap sum_c f(in[src(m,tap), c]) * W[tap][c][n] + bias[n]
 *   in_bnstate  NULL, or float[4*Cin] {scale, shift, mean, invstd}: f(x) = x*scale + shift, the
 *               BatchNormalization of the producing layer (:194,:204), then ReLU if LISEC_CONV_IN_RELU
 *               (:206); padding stays exactly zero, as ZeroPadding follows the activation in the graph
 *   bias        NULL or float[Cout]
 *   stats_partials NULL, or double[num_mblocks][2][Cout]: per-tile sum and sum of squares of the
 *               stored values, the input of lisec_bn_finalize (training-mode batch statistics)
 *   row_coords  NULL (dense: every position of the output map), or a ROW LIST: GEMM row m is the output
 *               position (d,h,w) = row_coords[3m..3m+2] (the voxeliser's `coords`), *row_count rows exist
 *               (device int, <= row_capacity) and out row m is written compactly at out + m*out_stride.
 *               Used to evaluate the gradient of the dense VFE grid only at occupied cells.
 *   workspace   NULL, or scratch of lisec_conv_forward_workspace_bytes(g): lets layers with few output
 *               positions (RPN blocks 2-3) be cut into K slices so that they still fill the 256 CUs; the
 *               slices are combined in a fixed order (deterministic).  With a row list the plan is made for
 *               row_capacity rows: size the scratch with lisec_conv_forward_rows_workspace_bytes.
 */
size_t lisec_conv_forward_workspace_bytes(const lisec_conv_geom* g);
size_t lisec_conv_forward_rows_workspace_bytes(const lisec_conv_geom* g, int row_capacity);
/* The workspace of the contraction entry points must be ZERO-FILLED once, before its first use: it starts with the
 * arrival counters of the K slices (the slices of a tile are combined inside the kernel by the last one to arrive, in
 * slice order -- deterministic, no combine launch), which every call leaves at zero.  One workspace serves any number of
 * layers on ONE stream; calls that may overlap on two streams need a workspace each. */
/* lisec_conv_forward with optional extras (NULL fields = off):
 *   out_mask     the output gate of lisec_conv_forward_masked
 *   bwd_y, bwd_bnstate, bwd_relu
 *                the call computes a gradient dA that is about to cross a BatchNormalization(+ReLU) backwards:
 *                bwd_y is that layer's raw output (positions x Cout, row stride Cout), bwd_bnstate its bnstate.
 *                stats_partials (required; lisec_conv_num_mblocks_bwd(g) rows) then receives per tile
 *                (sum dz, sum dz*yhat), dz = dA * (bwd_relu ? bn(y) > 0 : 1), yhat = (y - mean)*invstd -- pass 1 of
 *                lisec_bn_backward, folded into the store; finish with lisec_bn_backward_apply. */
/* Optional destination of the per-tile BatchNormalization sums of a contraction (instead of the stats_partials
 * table + a lisec_bn_finalize / lisec_bn_backward_apply finaliser launch): the sums are added into order-independent
 * fixed-point accumulators and the LAST workgroup of the call finalises them in place -- deterministic, no extra launch.
 *   acc   device, lisec_bn_sink_words(Cout) int64 words, ZERO before the first use; every call leaves it zeroed
 *   kind  LISEC_SINK_FORWARD: (sum y, sum y^2) -> bnstate as lisec_bn_finalize writes it (+ moving statistics when
 *         moving_mean/moving_var are set)
 *         LISEC_SINK_BACKWARD (with bwd_y): (sum dz, sum dz*yhat) -> dgamma, dbeta and coef float[2*Cout] =
 *         (mean dz, mean dz*yhat), the input of lisec_bn_backward_apply_coef */
#define LISEC_SINK_FORWARD 1
#define LISEC_SINK_BACKWARD 2
typedef struct lisec_bn_sink {
    void* acc;
    int kind;
    int unbiased_moving;
    double n_rows;
    const float* gamma;
    const float* beta;
    float* moving_mean;
    float* moving_var;
    float* bnstate;
    float* dgamma;
    float* dbeta;
    float* coef;
} lisec_bn_sink;
size_t lisec_bn_sink_words(int C);

typedef struct lisec_conv_extras {
    const float* out_mask;
    const float* bwd_y;
    const float* bwd_bnstate;
    int bwd_relu;
    const lisec_bn_sink* sink;
    /* optional, row-list calls: int32[2] device words, ZERO before the first use (every call leaves them zero).  With them a
     * row list whose capacity is large (>= 768 tiles of 128 rows) and whose Cout <= 64 runs as resident workgroups that
     * draw their tiles from a counter -- the tiles of a row list do very unequal work (rows beyond the device-side count,
     * depth parity), which one workgroup per tile turns into idle CUs. */
    int32_t* queue;
    /* optional second contraction riding on the stored tile (model_training.py:195, backwards: the gradient this call stores
     * is the one w.r.t. a middle block's Dense(64, relu) output, gated by out_mask; the Dense's own data gradient is one more
     * 64 x 64 contraction of the same rows):  tail_out[m, :] = out[m, :] (as stored) @ tail_w,  tail_w a packed 64 x 64 kernel
     * (lisec_conv_pack_weights), tail_out (positions, 64).  bwd_y / bwd_bnstate / bwd_relu / sink then describe tail_out.
     * Needs the two-line w-halo kernel (3 taps along w, stride 1, Wo >= 126), Cout = out_stride = 64; LISEC_EINVAL otherwise. */
    const float* tail_w;
    float* tail_out;
    /* optional BatchNormalization-backward APPLY ON LOAD (model_training.py:204-206 backwards): `in` is a gradient w.r.t. the
     * output of BatchNormalization(+ReLU) over the raw map in_y (same layout as `in`), whose backward statistics a sink has
     * already finalised: every gathered element becomes  scale * (gate(y) * g - mean(dz) - yhat * mean(dz * yhat))  -- what
     * lisec_bn_backward_apply_coef would have written -- so the data gradient of a layer runs straight behind the one above it.
     * in_fold_bnstate: the layer's bnstate float[4*Cin]; in_fold_coef: float[2*Cin] (lisec_bn_sink.coef); in_fold_relu: gate.
     * Transposed gathers (mode 1) without in_bnstate / LISEC_CONV_IN_RELU only. */
    const float* in_y;
    const float* in_fold_bnstate;
    const float* in_fold_coef;
    int in_fold_relu;
    /* optional weight gradient of the SAME Dense (model_training.py:195 backwards, what fit() derives for its kernel, :299),
     * for the call that is a Dense(64)'s data gradient with backward statistics (1x1x1, 64 -> 64, packed rows, bwd_y + a
     * LISEC_SINK_BACKWARD sink, no in_bnstate): the call already reads both operands of
     *     dW[i][j] = sum_m f(bwd_y[m, i]) * in[m, j],   f = bwd_bnstate's affine (+ ReLU when bwd_relu)
     * -- the Dense's input is the BatchNormalization output whose statistics the call reduces -- so the resident workgroups
     * accumulate it beside the data gradient instead of a second pass over 2 x (positions x 64) floats.
     * dense_dw: lisec_dense_dw_slabs() x 4096 floats, 16-byte aligned, no initialisation needed; lisec_dense_dw_reduce then
     * sums the slabs in index order (deterministic) into dW (64, 64) = (in channel, out channel), the Keras layout.
     * Needs at least lisec_dense_dw_slabs() tiles of 128 rows; LISEC_EINVAL for any other call. */
    float* dense_dw;
} lisec_conv_extras;
int lisec_dense_dw_slabs(void);
int lisec_dense_dw_reduce(const float* slabs, float* dW, lisec_stream_t stream);
int lisec_conv_num_mblocks_bwd(const lisec_conv_geom* g);

/* The launch plan lisec_conv_forward_ex WILL run for these arguments (pointers only matter as NULL / non-NULL, so the
 * query takes flags for them): which kernel, the workgroup shape, the K slicing, the row order.  Tests pin the plans of
 * the Lyft layer geometries with it; nothing is launched. */
enum { LISEC_KERNEL_IGEMM = 0,   /* generic gather, 128 x 64 tile                                             */
       LISEC_KERNEL_HALO2 = 1,   /* w-halo staging, at most two output lines per tile (Wo >= 126)             */
       LISEC_KERNEL_HALO3 = 2,   /* w-halo staging, three lines per tile (64 <= Wo < 126)                     */
       LISEC_KERNEL_DENSE64 = 3, /* resident workgroups, 1x1 64 -> 64                                         */
       LISEC_KERNEL_QUEUE = 4,   /* resident workgroups drawing row-list tiles from a counter                 */
       LISEC_KERNEL_WIDE = 5 };  /* 128 x 128 tiles, 512-thread workgroups, two-line w-halo staging           */
typedef struct lisec_conv_plan {
    int kernel;          /* LISEC_KERNEL_*                                                                    */
    int cols;            /* output columns per workgroup: 64, 32 (instead of two K slices) or 128 (wide tile) */
    int tiles;           /* tiles of the call, of tile_rows rows (parity-class order pads every class to whole tiles) */
    int tail_tile0;      /* first tile of the K-sliced tail (0: the whole layer is sliced, == tiles: none)    */
    int k_slices;        /* K slices of the tail, combined in-kernel by the last slice to arrive              */
    int plane_pair;      /* one workgroup per pair of depth planes                                            */
    int parity_classes;  /* rows visited in (h & 1, w & 1) classes (data gradient of a stride-2 Conv2D)       */
    int workgroups, launches;
    int double_buffered; /* the K-sliced launch runs the two-image kernels, one workgroup per CU              */
    int tile_rows;       /* rows per tile: 128, or 64 (LISEC_CONV_SMALL_TILE honoured: two workgroups per CU)   */
} lisec_conv_plan;
int lisec_conv_plan_query(const lisec_conv_geom* g, int has_in_bnstate, int flags, const lisec_conv_extras* extras,
                          int has_stats_table, size_t workspace_bytes, int has_row_list, int row_capacity,
                          lisec_conv_plan* plan);
int lisec_conv_forward_ex(const lisec_conv_geom* g, const float* in, const float* packed_w, const float* bias,
                          const float* in_bnstate, int flags, float* out, const lisec_conv_extras* extras,
                          double* stats_partials, void* workspace, size_t workspace_bytes,
                          const int32_t* row_coords, const int32_t* row_count, int row_capacity,
                          lisec_stream_t stream);
/* lisec_conv_forward with an output gate: stored value = out_mask[m][n] > 0 ? value : 0, out_mask laid out like
 * `out` (same stride).  The data gradient of a layer whose consumer-side activation was a ReLU is gated by that
 * activation while it is stored (what lisec_relu_mask does in a separate pass).  out_mask NULL = no gate. */
int lisec_conv_forward_masked(const lisec_conv_geom* g, const float* in, const float* packed_w, const float* bias,
                              const float* in_bnstate, int flags, float* out, const float* out_mask,
                              double* stats_partials, void* workspace, size_t workspace_bytes,
                              const int32_t* row_coords, const int32_t* row_count, int row_capacity,
                              lisec_stream_t stream);
int lisec_conv_forward(const lisec_conv_geom* g, const float* in, const float* packed_w, const float* bias,
                       const float* in_bnstate, int flags, float* out, double* stats_partials,
                       void* workspace, size_t workspace_bytes, const int32_t* row_coords,
                       const int32_t* row_count, int row_capacity, lisec_stream_t stream);

/* Winograd F(2x2, 3x3) form of lisec_conv_forward_ex (csrc/wino.hip) for contractions with 3 x 3 (h, w) taps, stride 1 and
 * padding 1 along h and w, any depth taps / depth stride, both gather modes: the Conv3D middle blocks
 * (model_training.py:193, 237-238), the stride-1 Conv2Ds of the RPN (:210-214) and the data gradients of both.  Same
 * arithmetic contract as lisec_conv_forward_ex -- fp32 operands, fp32 accumulation, in_bnstate / LISEC_CONV_IN_RELU applied
 * on load with exact zero padding, bias, LISEC_CONV_ACCUMULATE / LISEC_CONV_OUT_RELU, extras.out_mask, extras.bwd_y +
 * a LISEC_SINK_BACKWARD sink, or a LISEC_SINK_FORWARD sink, extras.tail_w / tail_out (Cout = out_stride = 64) -- with 4 / 9 of the multiplications: a 2 x 2 block of outputs is
 * A^T [ sum_c (G g G^T) . (B^T d B) ] A.  Results differ from lisec_conv_forward_ex by fp32 rounding only (the transforms add
 * and halve exactly representable values; tests/test_gpu_winograd.py holds both against the fp64 oracle).
 *   lisec_conv_pack_weights_winograd: G g G^T of every (depth tap, k, n) kernel slice, in the LDS image order of the kernel.
 *       src element (tap, k, n), tap = (kd * 3 + kh) * 3 + kw, is read at src[tap*tap_stride + k*k_stride + n*n_stride];
 *       flip_hw != 0 mirrors the (kh, kw) taps -- the data gradient of a stride-1 correlation is the correlation with the
 *       mirrored kernel and K / N swapped (k_stride / n_stride), so g->mode == 1 calls take a kernel packed with flip_hw = 1.
 *       dst: lisec_conv_winograd_packed_floats(KD, K, N) floats, 16-byte aligned.
 *   lisec_conv_winograd_supported: 1 when lisec_conv_forward_winograd serves these arguments (extras: only the fields named
 *       above; statistics only through a sink; Cin % 8 == 0), else 0 -- nothing is launched.
 *   lisec_conv_forward_winograd: no workspace (never K-sliced); LISEC_EINVAL for arguments it does not serve. */
size_t lisec_conv_winograd_packed_floats(int KD, int K, int N);
int lisec_conv_pack_weights_winograd(const float* src, int KD, int K, int N, long long tap_stride, long long k_stride,
                                     long long n_stride, int flip_hw, float* dst, lisec_stream_t stream);
int lisec_conv_winograd_supported(const lisec_conv_geom* g, int has_in_bnstate, int flags, const lisec_conv_extras* extras);
int lisec_conv_forward_winograd(const lisec_conv_geom* g, const float* in, const float* wino_w, const float* bias,
                                const float* in_bnstate, int flags, float* out, const lisec_conv_extras* extras,
                                lisec_stream_t stream);

/* Inference forward on the bf16 matrix cores (csrc/igemm_bf16.hip, v_mfma_f32_32x32x16_bf16): what the 'mixed_bfloat16'
 * policy runs for the Conv3D blocks behind the first (model_training.py:237-238) and the Conv2Ds of the RPN (:203).
 *   out[m, n] = sum_tap sum_c bf16(f(in[src(m,tap), c])) * bf16(W[tap][c][n]) + bias[n]
 * `in`, `out`, bias and in_bnstate are the fp32 buffers of lisec_conv_forward, in the same layouts; f (the affine of
 * in_bnstate, then ReLU if LISEC_CONV_IN_RELU) is evaluated in fp32 as one fma, its result and the kernel are rounded to
 * bf16 to nearest-even, products are accumulated in fp32, and bias / LISEC_CONV_OUT_RELU are fp32: relative to the fp32
 * contraction the result carries the two operand roundings (2^-9 each) and nothing else.  Padding stays exactly zero.
 *   lisec_conv_packed_bf16_bytes / lisec_conv_pack_weights_bf16: the layout the kernel reads, [tap][K/8][N][8] bf16 with K
 *       and N zero padded to 64, from src[tap*tap_stride + k*k_stride + n*n_stride] (fp32, as lisec_conv_pack_weights);
 *       dst 16-byte aligned.
 *   lisec_conv_forward_bf16: g->mode == 0, no pixel-shuffle store, dense rows, flags within IN_RELU | OUT_RELU (IN_RELU
 *       needs in_bnstate); LISEC_EINVAL for anything else -- it never runs the fp32 kernels instead.  No statistics.
 *       workspace: NULL, or lisec_conv_forward_bf16_workspace_bytes(g) bytes under the rules of the lisec_conv_forward
 *       workspace (zero-filled once, one per stream; it may be the same buffer): layers of fewer tiles than CUs are cut
 *       into K slices that meet in slice order inside the kernel (deterministic).  A smaller workspace means fewer slices. */
size_t lisec_conv_packed_bf16_bytes(int ntaps, int K, int N);
int lisec_conv_pack_weights_bf16(const float* src, int ntaps, int K, int N, long long tap_stride, long long k_stride,
                                 long long n_stride, void* dst, lisec_stream_t stream);
size_t lisec_conv_forward_bf16_workspace_bytes(const lisec_conv_geom* g);
int lisec_conv_forward_bf16(const lisec_conv_geom* g, const float* in, const void* packed_bf16, float* out, const float* bias,
                            const float* in_bnstate, int flags, void* workspace, size_t workspace_bytes,
                            lisec_stream_t stream);

/* Winograd F(2x2, 3x3) form of lisec_conv_wgrad (csrc/wino_wgrad.hip) for the 64 -> 64 Conv3D blocks with 3 x 3 (h, w) taps, stride 1
 * and padding 1 along h and w (model_training.py:193, 237-238; what fit() derives for their kernels, :299): dU[kd] = sum over
 * tiles of (B^T d B) (x) (A dY A^T) per transform point, then dW = G^T dU G -- 4 / 9 of the multiplications of the direct weight
 * gradient, fp32 operands and accumulation, slabs summed in a fixed order (deterministic).  g: the geometry of the FORWARD layer
 * (mode 0), in = the layer's input (packed rows of 64), dy (packed rows of 64), dW in the Keras layout (taps, 64, 64).  No
 * on-load affine.  workspace: lisec_conv_wgrad_winograd_workspace_bytes(g), no initialisation needed. */
int lisec_conv_wgrad_winograd_supported(const lisec_conv_geom* g);
size_t lisec_conv_wgrad_winograd_workspace_bytes(const lisec_conv_geom* g);
int lisec_conv_wgrad_winograd(const lisec_conv_geom* g, const float* in, const float* dy, void* workspace,
                              size_t workspace_bytes, float* dW, lisec_stream_t stream);

/* Weight gradient of the contraction described by `g` (the geometry of the FORWARD layer):
 *   dW[tap][c][n] = sum_m f(in[src(m,tap), c]) * dy[m, n]      dy: float32, g->out_stride floats per row
 * Written in the Keras kernel layout (taps, Cin, Cout); transpose_out != 0 writes (taps, Cout, Cin),
 * the Conv2DTranspose layout (kh,kw,out,in).  dy_bnstate (optional, float[4*Cout]) applies the same
 * affine (+ReLU with LISEC_CONV_DY_RELU) to the dy operand: the kernel==stride Conv2DTranspose layers
 * swap roles (in = gathered output gradient, dy = the layer's BN+ReLU input).
 * row_coords/row_count/row_capacity (optional): contraction over a ROW LIST instead of every position: row m
 * is position row_coords[3m..], `in` is gathered there, dy row m is read at dy + m*out_stride.
 * Deterministic: partial slabs reduced in index order. */
size_t lisec_conv_wgrad_workspace_bytes(const lisec_conv_geom* g, int row_capacity);
/* The launch plan lisec_conv_wgrad WILL run (nothing is launched): tests pin the plans of the Lyft layer geometries. */
typedef struct lisec_wgrad_plan {
    int halo;            /* w-halo kernel (3 taps along w at stride 1 over every position): tiles follow the output lines */
    int mirrored;        /* a unit-stride transposed gather run as the plain one with mirrored taps                       */
    int taps_per_group;  /* taps that share one staged dy tile                                                           */
    int groups;          /* tap groups that get workgroups (groups no output line can read are left out)                  */
    int tile_rows;       /* rows per staged tile (halo: equal tiles per output line)                                      */
    int staging_passes;  /* halo: 7 (tiles of <= 104 rows, three workgroups per CU) or 9                                  */
    int tiles, slabs, tiles_per_slab;   /* M tiles, partial slabs (= ranges of tiles), tiles per range                   */
    int workgroups;
    int lane_reduce;     /* >= 32 slabs summed by a separate launch: the lane-strided slab sum                            */
    int combine_in_kernel; /* few slabs per cell: summed by the last slice to arrive, no slab-sum launch                  */
    int ring;            /* ring kernel (3 x 3 taps in (h, w) at stride 1): one 768-thread workgroup owns a run of output  */
                         /* lines of one (cell, kd, plane, w segment) column and all nine taps; the three input lines live */
                         /* in an LDS ring, so x and dy are staged once per nine taps.  groups = (kd, plane) pairs,        */
                         /* taps_per_group = 9, staging_passes = 48-row passes (2 or 3), slabs = most slices of a cell     */
    int runs_per_column; /* ring: runs every column of Ho output lines is cut into                                        */
    int lines_per_run;   /* ring: most output lines of a run                                                               */
} lisec_wgrad_plan;
int lisec_conv_wgrad_plan_query(const lisec_conv_geom* g, int flags, int has_dy_bnstate, int has_row_list, int row_capacity,
                                lisec_wgrad_plan* plan);
int lisec_conv_wgrad(const lisec_conv_geom* g, const float* in, const float* in_bnstate, int flags,
                     const float* dy, const float* dy_bnstate, void* workspace, size_t workspace_bytes,
                     int transpose_out, float* dW, const int32_t* row_coords, const int32_t* row_count,
                     int row_capacity, lisec_stream_t stream);
/* The weight-gradient workspace must be ZERO-FILLED once before its first use, like the contraction workspace: contractions
 * whose slabs are combined inside the kernel keep their arrival counters at its head (left at zero by every call).
 *
 * Several weight gradients in ONE launch: the stride-1 3x3 convolutions of an RPN block (:203, three to five layers whose
 * maps hold 1 250 - 20 000 positions) fill a fraction of the chip each and are leaves of the backward pass, so they can wait
 * for each other and share a launch.  Items that cannot share one (not all on the w-halo kernel with the same staging) run
 * one after the other with the same results.  n <= 6. */
typedef struct lisec_wgrad_item {
    const lisec_conv_geom* g;
    const float* in;
    const float* in_bnstate;
    int flags;
    const float* dy;
    int transpose_out;
    float* dW;
} lisec_wgrad_item;
size_t lisec_conv_wgrad_batched_workspace_bytes(const lisec_wgrad_item* items, int n);
int lisec_conv_wgrad_batched(const lisec_wgrad_item* items, int n, void* workspace, size_t workspace_bytes,
                             lisec_stream_t stream);

/* First middle layer, exact sparse backward (see csrc/sparse_grid.hip).
 *   lisec_conv_tap_sums: S[tap][n] = sum of dy[m][n] over the output positions m of the mode-0 conv `g` whose
 *     tap reads inside the input map; S: float[ntaps*Cout].
 *   lisec_const_field_grads: for an input map equal to the constant vector cvec (Cin) everywhere,
 *     g_all[c] = sum_tap sum_n W[tap][c][n]*S[tap][n]  (sum of the data gradient over ALL input positions)
 *     dW[tap][c][n] += cvec[c]*S[tap][n]               (W, dW: Keras layout (taps, Cin, Cout); either output
 *     may be NULL).  cvec_row (optional, device int): the constant is row min(*cvec_row, cvec_row_max) of the
 *     (rows, Cin) table `cvec` -- the voxel count V only exists on the device. */
size_t lisec_conv_tap_sums_workspace_bytes(const lisec_conv_geom* g);
int lisec_conv_tap_sums(const lisec_conv_geom* g, const float* dy, float* S, void* workspace,
                        size_t workspace_bytes, lisec_stream_t stream);
/* lisec_conv_tap_sums fused with the apply pass of the BatchNormalization backward in front of it (what
 * lisec_bn_backward_apply_coef(relu = 0) computes): dz is the gradient of the normalised map, y / bnstate / coef as
 * there; dy = scale * (dz - coef[c] - yhat * coef[C + c]) is stored (dy may alias dz, row stride Cout) and S is
 * summed over dy -- one pass over the map instead of two. */
int lisec_conv_tap_sums_bn(const lisec_conv_geom* g, const float* dz, const float* y, const float* bnstate,
                           const float* coef, float* dy, float* S, void* workspace, size_t workspace_bytes,
                           lisec_stream_t stream);
/* S == NULL in lisec_conv_tap_sums_bn stops after the per-line sums (left in `workspace`); lisec_conv_tap_sums_finish sums
 * them into S later -- on another stream, beside the row-list data gradient that only needs the dy the first pass stored. */
int lisec_conv_tap_sums_finish(const lisec_conv_geom* g, const void* workspace, size_t workspace_bytes, float* S,
                               lisec_stream_t stream);
int lisec_const_field_grads(const float* W, const float* S, const float* cvec, const int32_t* cvec_row,
                            int cvec_row_max, int ntaps, int Cin, int Cout, float* dW, float* g_all,
                            lisec_stream_t stream);

/* First middle layer, forward over the VFE's compact output instead of the dense grid (csrc/field_conv.hip): the tensor
 * Conv3D(64, 3, (2,1,1)) reads at model_training.py:236 is a constant vector on the empty cells plus V voxel rows, so
 *   out[p] = bias + sum_{taps inside the grid} W[tap]^T c + sum_{taps that read voxel v} W[tap]^T delta_v
 * is evaluated as one V x 64 x (27*64) contraction and one pass that writes `out` -- the same values as
 * lisec_conv_forward on the dense grid up to fp32 summation order, ~1 GFLOP instead of 70.8 on a Lyft sweep.
 *   g          mode-0 geometry of the layer, Cin == Cout == 64, at most 3 taps per axis
 *   vout/delta the VOUT / DELTA fields of lisec_vfe_forward's `saved` buffer ((row_capacity+1, 64) each)
 *   info, coords, cell_voxel: the voxeliser's outputs; row_capacity: its voxel capacity
 *   packed_w   the layer's kernel from lisec_conv_pack_weights (the layout lisec_conv_forward takes)
 *   out        float32 (Do*Ho*Wo, out_stride), every row written
 *   sink       optional LISEC_SINK_FORWARD sink: BatchNormalization batch statistics of `out`, finalised in the call
 * Deterministic (every sum in a fixed order, statistics in fixed-point accumulators). */
size_t lisec_conv_field_forward_workspace_bytes(const lisec_conv_geom* g, int row_capacity);
int lisec_conv_field_forward(const lisec_conv_geom* g, const float* vout, const float* delta, const int32_t* info,
                             const int32_t* coords, const int32_t* cell_voxel, int row_capacity,
                             const float* packed_w, const float* bias, float* out, const lisec_bn_sink* sink,
                             void* workspace, size_t workspace_bytes, lisec_stream_t stream);

/* Upsampling branches + heads collapsed into 16-channel contractions (csrc/head_fused.hip).  The three
 * Conv2DTranspose layers (model_training.py:246,249,252) carry a bias but no BatchNormalization and no activation, and the
 * two 1x1 heads (:254-255) read their Concatenate (:253) linearly, so
 *     head[m][j] = b'_j + sum_b sum_{tap,c} x_b[src_b(m,tap)][c] * Wc_b[tap][c][j],
 *     Wc_b[tap][c][j] = sum_n W_b[tap][n][c] * H[256 b + n][j],   b'_j = b_j + sum_b sum_n bias_b[n] * H[256 b + n][j]
 * (W_b: the Keras Conv2DTranspose kernel (kh,kw,out,in); H = [W_cls | W_reg], (768,16)): transposed convolutions to 16
 * channels through lisec_conv_forward instead of three to 256 channels and a 768 -> 16 contraction; the (100,200,768)
 * concat tensor and its gradient are never formed.  Same values up to fp32 summation order.
 *   lisec_head_compose: Wc[tap*out_tap_stride + c*out_c_stride + j] (j < 16) for ONE branch; head_w = the 256 rows of H
 *     that branch feeds ((Cup,16), row stride 16); bias_out[j] = (bias_in ? bias_in[j] : 0) + sum_n up_bias[n]*H[n][j]
 *     (bias_out NULL: skipped; chain the branches through bias_in, starting from the heads' own bias).
 *   lisec_head_compose_backward: from G = dL/dWc (same indexing as Wc; the lisec_conv_wgrad of the 16-channel contraction)
 *     and S[j] = sum_m dhead[m][j]:  d_up_kernel (taps,Cup,Cin), d_up_bias (Cup), d_head_w (Cup,16) of that branch
     (d_head_w includes up_bias[n]*S[j]: the branch carries its bias into the heads).
 *   lisec_head_shuffle: the kernel == stride branches run as 1x1 contractions with columns (tap, j):
 *     T_b[pos][tap*16 + j], pos = (h/ps_b)*(Wo/ps_b) + w/ps_b, tap = (h%ps_b)*ps_b + w%ps_b, over the (Ho,Wo,16) head map.
 *     backward == 0: head[m][j] += sum_b T_b[...];  backward != 0: T_b[...] = head[m][j] (head = dL/dhead, T_b = dL/dT_b).
 *     T, ps: HOST arrays of n_branches (<= 4) device pointers / strides. */
int lisec_head_compose(const float* up_kernel, const float* up_bias, const float* head_w, int taps, int Cin, int Cup,
                       long long out_tap_stride, long long out_c_stride, float* Wc, const float* bias_in, float* bias_out,
                       lisec_stream_t stream);
int lisec_head_compose_backward(const float* G, long long g_tap_stride, long long g_c_stride, const float* up_kernel,
                                const float* up_bias, const float* head_w, const float* S, int taps, int Cin, int Cup,
                                float* d_up_kernel, float* d_up_bias, float* d_head_w, lisec_stream_t stream);
int lisec_head_shuffle(float* head, int Ho, int Wo, int n_branches, float* const* T, const int* ps, int backward,
                       lisec_stream_t stream);

/* BatchNormalization statistics (Keras: axis -1, eps 1e-3, momentum 0.99, biased batch variance).
 * bnstate: float[4*C] {scale = gamma*rsqrt(var+eps), shift = beta - mean*scale, mean, invstd}.
 * finalize: reduces partials in index order, optionally updates the moving statistics in place
 * (NULL to skip); fold: bnstate from the moving statistics (inference, Predict.py:38). */
int lisec_bn_finalize(const double* partials, int nparts, int C, double n_rows, const float* gamma,
                      const float* beta, float* moving_mean, float* moving_var, int unbiased_moving,
                      float* bnstate, lisec_stream_t stream);
int lisec_bn_fold(const float* gamma, const float* beta, const float* moving_mean, const float* moving_var,
                  int C, float* bnstate, lisec_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * 4. Training-step helpers (what Keras' fit() does around the contractions, model_training.py:295-299)
 * ------------------------------------------------------------------------------------------ */
size_t lisec_eltwise_workspace_bytes(void);

/* Backward of BatchNormalization (training mode) optionally followed by ReLU (:171-173, :194, :204-206).
 *   dA (M rows, da_stride floats apart, C channels): gradient wrt the activation a = [relu](y*scale+shift)
 *   y  (M, C) raw pre-BN values; bnstate from the forward's lisec_bn_finalize
 *   dz = dA * [z > 0];  dbeta = sum dz;  dgamma = sum dz*yhat;
 *   dy = scale * (dz - dbeta/M - yhat*dgamma/M)           (may alias dA when da_stride == C)
 *   dbias (optional): sum over rows of dy -- the gradient of the bias of the conv that produced y */
int lisec_bn_backward(const float* dA, int da_stride, const float* y, const float* bnstate, long long M, int C,
                      int relu, float* dgamma, float* dbeta, float* dbias, float* dy, void* workspace,
                      size_t workspace_bytes, lisec_stream_t stream);
/* Passes 2-3 of lisec_bn_backward for a gradient whose pass-1 partials (sum dz, sum dz*yhat per tile) were produced by
 * lisec_conv_forward_ex: sums `partials` (double[nparts][2][C], index order), writes dgamma / dbeta and
 * dy = scale * (dz - mean(dz) - yhat * mean(dz*yhat)); dy may alias dA. */
int lisec_bn_backward_apply(const float* dA, int da_stride, const float* y, const float* bnstate, long long M, int C,
                            int relu, const double* partials, int nparts, float* dgamma, float* dbeta, float* dy,
                            void* workspace, size_t workspace_bytes, lisec_stream_t stream);

/* The apply pass alone, for coefficients a lisec_bn_sink (LISEC_SINK_BACKWARD) produced: coef float[2*C] =
 * (mean dz, mean dz*yhat); dy = scale * (dz - coef[c] - yhat * coef[C + c]); dy may alias dA. */
int lisec_bn_backward_apply_coef(const float* dA, int da_stride, const float* y, const float* bnstate, long long M, int C,
                                 int relu, const float* coef, float* dy, lisec_stream_t stream);

/* n strided 2-D float copies in one launch: dst[r*dst_stride + c] = src[r*src_stride + c], r < rows, c < cols.
 * `device_table` lives in device memory (the pointers are fixed for the life of a model). */
typedef struct lisec_copy_desc {
    const float* src;
    float* dst;
    int rows, cols;
    long long src_stride, dst_stride;
} lisec_copy_desc;
int lisec_copy2d_batched(const lisec_copy_desc* device_table, int n, lisec_stream_t stream);

/* Permute((2,3,4,1)) + Reshape (model_training.py:242-243): in (D,H,W,C) -> out (H,W,C*D), channel c*D + d; HW = H*W.
 * With the reference's Constants.nz = 8 the depth is 1 there and the fold is a view; other nz need this copy.
 * inverse != 0: out (D,H,W,C) <- in (H,W,C*D), the gradient's way back, stored as 0 where mask (laid out like out,
 * optional) is <= 0 -- the ReLU of the Dense layer that produced the folded tensor. */
int lisec_fold_depth(const float* in, float* out, int D, long long HW, int C, int inverse, const float* mask,
                     lisec_stream_t stream);

/* grad[i] = act[i] > 0 ? grad[i] : 0   (backward of Dense(..., 'relu'), :195) */
int lisec_relu_mask(float* grad, const float* act, long long n, lisec_stream_t stream);

/* out[c] = sum_m x[m*stride + c]  (bias gradients of Conv2DTranspose / head layers); C divides 256, or is a
 * multiple of 256 up to 1024 (the 768-channel concat gradient in one pass) */
int lisec_colsum(const float* x, int stride, long long M, int C, float* out, void* workspace,
                 size_t workspace_bytes, lisec_stream_t stream);

/* head: (M,16) = [classification (2) | regression (14)] maps.  kind 0: loss=['mse','mse'] (:296);
 * kind 1: sigmoid cross-entropy + SmoothL1 (BASELINE config 4).  Writes dhead = grad_scale * dLoss/dhead and
 * loss_out[3] = {total, class, regression}. */
int lisec_rpn_loss(const float* head, const float* y_cls, const float* y_reg, long long M, int kind,
                   float grad_scale, float* dhead, float* loss_out, void* workspace, size_t workspace_bytes,
                   lisec_stream_t stream);

/* The evaluation loss (Model.evaluate, validation in fit): the [total, class, regression] lisec_rpn_loss writes to
 * loss_out for the same inputs, bit for bit, without a gradient.  They are ADDED, as doubles, to acc[0..2], and acc[3] is
 * incremented (the number of sweeps); acc (double[4], device) is zeroed by the caller.  No atomics: deterministic. */
int lisec_rpn_loss_eval(const float* head, const float* y_cls, const float* y_reg, long long M, int kind, double* acc,
                        void* workspace, size_t workspace_bytes, lisec_stream_t stream);

/* tf.keras 2.4 losses and metrics of Model.compile(loss=, loss_weights=, metrics=) on the two head outputs (csrc/losses.hip).
 * With e = p - t, eps = 1e-7, every term is a mean over all M*C elements of the output (C = 2 class, 14 regression):
 *   MSE e^2 | MAE |e| | MAPE 100|t-p|/max(|t|,eps) | MSLE (log(max(p,eps)+1) - log(max(t,eps)+1))^2
 *   HUBER |e| <= delta ? e^2/2 : delta^2/2 + delta(|e| - delta) | LOGCOSH e + softplus(-2e) - log 2
 *   BCE t <- t(1-ls) + ls/2; from_logits: max(p,0) - p t + log1p(exp(-|p|)), else o = clip(p, eps, 1-eps),
 *       -(t log(o+eps) + (1-t) log(1-o+eps)) | POISSON p - t log(p+eps)
 *   SIGMOID_CE_CLAMPED, SMOOTH_L1: the two halves of lisec_rpn_loss kind 1, with its fp32 arithmetic
 *   BINARY_ACCURACY (metric) t == (p > threshold) | CATEGORICAL_ACCURACY (metric, a mean over the M cells)
 *       argmax(t) == argmax(p) over the C channels of a cell, the first index winning ties
 * Labels are not clamped (except by SIGMOID_CE_CLAMPED).  Gradients are TF's of the same formulas. */
#define LISEC_LOSS_MAX_METRICS 4
enum {
    LISEC_LOSS_MSE = 0,
    LISEC_LOSS_MAE = 1,
    LISEC_LOSS_MAPE = 2,
    LISEC_LOSS_MSLE = 3,
    LISEC_LOSS_HUBER = 4,
    LISEC_LOSS_LOGCOSH = 5,
    LISEC_LOSS_BCE = 6,
    LISEC_LOSS_POISSON = 7,
    LISEC_LOSS_SIGMOID_CE_CLAMPED = 8,
    LISEC_LOSS_SMOOTH_L1 = 9,
    LISEC_METRIC_BINARY_ACCURACY = 10,   /* metrics only */
    LISEC_METRIC_CATEGORICAL_ACCURACY = 11
};
typedef struct lisec_loss_term {
    int kind;                 /* LISEC_LOSS_* / LISEC_METRIC_* */
    int from_logits;          /* BCE */
    float param;              /* HUBER: delta (> 0); BINARY_ACCURACY: threshold */
    float label_smoothing;    /* BCE, in [0, 1] */
} lisec_loss_term;
typedef struct lisec_loss_cfg {
    lisec_loss_term loss[2];                              /* [0] class output, [1] regression output */
    float weight[2];                                      /* loss_weights */
    int n_metrics[2];                                     /* 0 .. LISEC_LOSS_MAX_METRICS */
    lisec_loss_term metric[2][LISEC_LOSS_MAX_METRICS];
} lisec_loss_cfg;

/* One pass over head (M,16), y_cls (M,2), y_reg (M,14): dhead = grad_scale * d(weight[0]*L_cls + weight[1]*L_reg)/dhead,
 * loss_out[3] = {weight[0]*L_cls + weight[1]*L_reg, L_cls, L_reg} and metric_out[n_metrics[0] + n_metrics[1]] (the class
 * output's metrics, then the regression output's), fp32.  Per-workgroup fp64 partials in a fixed partition and one
 * finalize: no atomics, the same bits on every run.  metric_out may be NULL when there are no metrics.  With both losses
 * MSE at unit weights, dhead is bit-identical to lisec_rpn_loss kind 0 (and with SIGMOID_CE_CLAMPED + SMOOTH_L1, to kind 1). */
int lisec_head_loss(const lisec_loss_cfg* cfg, const float* head, const float* y_cls, const float* y_reg, long long M,
                    float grad_scale, float* dhead, float* loss_out, float* metric_out, void* workspace,
                    size_t workspace_bytes, lisec_stream_t stream);
/* The evaluation form: the same partition and finalize without the gradient, so that the values of a sweep are the bits
 * lisec_head_loss writes.  They are ADDED, as doubles, to acc = {total, class, regression, metrics..., sweeps} (device,
 * 4 + n_metrics[0] + n_metrics[1] doubles, zeroed by the caller); the last word counts the sweep. */
int lisec_head_loss_eval(const lisec_loss_cfg* cfg, const float* head, const float* y_cls, const float* y_reg, long long M,
                         double* acc, void* workspace, size_t workspace_bytes, lisec_stream_t stream);
size_t lisec_head_loss_workspace_bytes(void);

/* The VoxelNet detection loss (paper section 2.2; csrc/detection_loss.hip): one joint loss of both outputs on the label
 * code of lisec_rpn_labels / lisec_rpn_targets.  head (M,16): head[:, a] is the class logit z of anchor a (A = 2),
 * head[:, 2+7a+k] its regression output r.  y_cls (M,2): pos = code > 1.5, neg = 0.5 < code <= 1.5, anything else (0, a
 * NaN) is ignored.  y_reg (M,14): the targets, with the reference's +1 on positives (target_offset).  N_pos and N_neg are
 * the counts over the sweep; a count of 0 divides as 1.  With p = sigmoid(z), sp(x) = max(x,0) + log1p(exp(-|x|)):
 *   L_cls = alpha/N_pos sum_pos (1-p)^gamma sp(-z) + beta/N_neg sum_neg p^gamma sp(z)
 *   L_reg = 1/N_pos sum_pos sum_k S(r - (y_reg - target_offset)),  S(d) = |d| < b ? d*d/(2b) : |d| - b/2, b = smooth_l1_beta
 *   total = weight[0]*L_cls + weight[1]*L_reg
 * gamma = 0 is the paper's loss (the factor is exactly 1), gamma > 0 the focal form.  Every element is evaluated in double
 * from the fp32 inputs -- finite for every finite logit; a NaN logit gives NaN -- and summed in double over a fixed
 * partition with one finalize: no atomics, the same bits on every run. */
typedef struct lisec_detection_loss_cfg {
    int struct_bytes;           /* sizeof(lisec_detection_loss_cfg), checked */
    int reserved;               /* 0 */
    double alpha, beta, gamma;  /* >= 0 */
    double smooth_l1_beta;      /* > 0 */
    double target_offset;
    double weight[2];           /* loss_weights: class, regression */
} lisec_detection_loss_cfg;

/* dhead (M,16) = grad_scale * d total / d head -- exactly 0.0f on ignored anchors and on every regression channel of an
 * anchor that is not positive --, loss_out[3] = {total, L_cls, L_reg} (fp32) and counts_out[2] = {N_pos, N_neg} (device).
 * The counts come from a launch of their own over y_cls, ahead of the gradient they scale.  Fixed addresses, no host
 * reads: every launch records into a step plan.  LISEC_EINVAL: a NULL pointer, M <= 0, a negative alpha, beta or gamma,
 * smooth_l1_beta <= 0, a struct_bytes of another size, a workspace below lisec_detection_loss_workspace_bytes(). */
int lisec_detection_loss(const lisec_detection_loss_cfg* cfg, const float* head, const float* y_cls, const float* y_reg,
                         long long M, float grad_scale, float* dhead, float* loss_out, long long* counts_out,
                         void* workspace, size_t workspace_bytes, lisec_stream_t stream);
/* The evaluation form: the same launches without the gradient store, so a sweep's {total, L_cls, L_reg} are the fp32 bits
 * lisec_detection_loss writes.  They are ADDED, as doubles, to acc[0..2] and acc[3] counts the sweep (double[4], device,
 * zeroed by the caller), like lisec_rpn_loss_eval. */
int lisec_detection_loss_eval(const lisec_detection_loss_cfg* cfg, const float* head, const float* y_cls,
                              const float* y_reg, long long M, double* acc, void* workspace, size_t workspace_bytes,
                              lisec_stream_t stream);
size_t lisec_detection_loss_workspace_bytes(void);

/* The detection loss with a rotated-box IoU term beside SmoothL1 (csrc/detection_iou_loss.hip; ours).  Everything as for
 * lisec_detection_loss, except
 *   L_reg = 1/N_pos sum_pos [ sum_k S(r_k - t_k) + iou_weight (1 - IoU(decode(r), decode(t))) ],  t = y_reg - target_offset
 * with the decode and the IoU of the POSITIVE_IOU metric below: centre (r0 l_a, r1 w_a, r2 h_a), extents exp(r3..5) (l_a,
 * w_a, h_a), yaw r6 + yaw_a for the anchor (l_a, w_a, h_a, yaw_a) of the channel block; LISEC_IOU_BEV is the IoU of the
 * footprints, LISEC_IOU_3D multiplies by the clamped height overlap and divides by the volume of the union.  The target
 * box is a constant; the gradient of the term goes to the seven r of the positive anchor (under LISEC_IOU_BEV r2 and r5
 * get none) and is the exact derivative of the clipped area, added to the SmoothL1 derivative in double before the one
 * rounding.  IoU 0 -- a decoded box that is not finite, footprints or height intervals that do not meet -- adds
 * iou_weight to the sum and exactly +0.0 to the gradient, so such an anchor gets lisec_detection_loss's bits, and
 * iou_weight = 0 gives them everywhere.  The class channels, the counts and every anchor that is not positive are those
 * of lisec_detection_loss. */
typedef struct lisec_detection_iou_loss_cfg {
    int struct_bytes;               /* sizeof(lisec_detection_iou_loss_cfg), checked */
    int reserved;                   /* 0 */
    lisec_detection_loss_cfg det;   /* its own struct_bytes = sizeof(lisec_detection_loss_cfg), checked */
    double iou_weight;              /* >= 0, finite */
    int iou_mode;                   /* LISEC_IOU_3D / LISEC_IOU_BEV (lisec_boxes_match, below) */
    int reserved2;                  /* 0 */
    double anchors[2][4];           /* l, w, h, yaw: lisec_rpn_cfg's; extents > 0 */
} lisec_detection_iou_loss_cfg;

/* The argument lists of lisec_detection_loss*; one more launch (a thread per anchor) between the element pass and the
 * finalize.  loss_out[3] = {total, L_cls, L_reg} with the IoU term inside L_reg.  LISEC_EINVAL, with nothing enqueued:
 * lisec_detection_loss's refusals, a struct_bytes of another size, iou_weight negative or not finite, an unknown iou_mode,
 * an anchor that is not finite or has an extent <= 0. */
int lisec_detection_iou_loss(const lisec_detection_iou_loss_cfg* cfg, const float* head, const float* y_cls,
                             const float* y_reg, long long M, float grad_scale, float* dhead, float* loss_out,
                             long long* counts_out, void* workspace, size_t workspace_bytes, lisec_stream_t stream);
/* Adds the fp32 bits lisec_detection_iou_loss writes to acc[0..2], as doubles, and counts the sweep in acc[3]. */
int lisec_detection_iou_loss_eval(const lisec_detection_iou_loss_cfg* cfg, const float* head, const float* y_cls,
                                  const float* y_reg, long long M, double* acc, void* workspace, size_t workspace_bytes,
                                  lisec_stream_t stream);
size_t lisec_detection_iou_loss_workspace_bytes(void);     /* = lisec_detection_loss_workspace_bytes() */

/* Sample weights of fit(sample_weight=) / evaluate(sample_weight=) for the three loss families above (ours where tf.keras
 * 2.4 cannot be checked).  w_o[m] weighs cell m of output o (0 class, 1 regression): one device float for the sweep, or a
 * map of M floats.  The weights are read when the launch runs, so a recorded plan sees what was staged at the address.
 *   head loss:       L_o = 1/(M*C) sum_m w_o[m] sum_c v(m,c) -- the divisor stays the element count.  The fp32 kinds use
 *                    the gradient scale wf * w (one fp32 multiply), the fp64 kinds wd * (double)w; the sum adds (double)w * v.
 *   detection loss:  L_cls = alpha/N_pos sum_pos w_cls[m] (...) + beta/N_neg sum_neg w_cls[m] (...),
 *                    L_reg = 1/N_pos sum_pos w_reg[m] [sum_k S(...) + iou_weight (1 - IoU)]; N_pos and N_neg stay the
 *                    unweighted counts; the gradient scale is (wpos * (double)w), (wneg * (double)w), (wreg * (double)w).
 * A weight of exactly 1.0f gives the bits of the unweighted entry, a power of two scales dhead exactly.  A weight is a
 * factor, not a mask: 0 * NaN stays NaN, and a zero weight gives a zero gradient of either sign.
 * A weighted metric of the head loss (bit j of weighted_metrics[o]) is sum w*v / sum w over the elements of output o (over
 * its cells for CATEGORICAL_ACCURACY).  Every metric of a weighted head entry leaves as the fp64 pair {num, den}; den of an
 * unweighted metric is the element (cell) count.  The caller pools pairs and divides once (0 when den == 0). */
typedef struct lisec_sample_weights {
    int struct_bytes;               /* sizeof(lisec_sample_weights), checked */
    int per_cell[2];                /* 0: w[o] points at ONE float, the sweep's weight; 1: at M floats, one per cell */
    const float* w[2];              /* device; [0] class, [1] regression; NULL: that output has weight 1 */
    unsigned weighted_metrics[2];   /* head loss only: bit j = metric j of output o is weighted */
} lisec_sample_weights;

/* The argument lists of the unweighted entries with the descriptor behind cfg.  LISEC_EINVAL, with nothing enqueued and
 * every output untouched: the refusals of the unweighted entry, a NULL descriptor, a struct_bytes of another size, a
 * per_cell outside {0, 1}, a metric bit at or above n_metrics[o] (any metric bit, for the detection entries).
 * lisec_head_loss_weighted writes metric_pairs[2 * (n_metrics[0] + n_metrics[1])] = {num0, den0, ...} (device doubles, the
 * class output's metrics first); lisec_head_loss_weighted_eval ADDS to acc = {total, class, regression, sweeps, num0,
 * den0, ...} (4 + 2 * metrics doubles, zeroed by the caller): the fp32 losses as doubles, the pairs as they are.  The
 * detection entries keep the outputs of their twins. */
int lisec_head_loss_weighted(const lisec_loss_cfg* cfg, const lisec_sample_weights* sw, const float* head,
                             const float* y_cls, const float* y_reg, long long M, float grad_scale, float* dhead,
                             float* loss_out, double* metric_pairs, void* workspace, size_t workspace_bytes,
                             lisec_stream_t stream);
int lisec_head_loss_weighted_eval(const lisec_loss_cfg* cfg, const lisec_sample_weights* sw, const float* head,
                                  const float* y_cls, const float* y_reg, long long M, double* acc, void* workspace,
                                  size_t workspace_bytes, lisec_stream_t stream);
size_t lisec_head_loss_weighted_workspace_bytes(void);
int lisec_detection_loss_weighted(const lisec_detection_loss_cfg* cfg, const lisec_sample_weights* sw, const float* head,
                                  const float* y_cls, const float* y_reg, long long M, float grad_scale, float* dhead,
                                  float* loss_out, long long* counts_out, void* workspace, size_t workspace_bytes,
                                  lisec_stream_t stream);
int lisec_detection_loss_weighted_eval(const lisec_detection_loss_cfg* cfg, const lisec_sample_weights* sw,
                                       const float* head, const float* y_cls, const float* y_reg, long long M, double* acc,
                                       void* workspace, size_t workspace_bytes, lisec_stream_t stream);
size_t lisec_detection_loss_weighted_workspace_bytes(void);        /* = lisec_detection_loss_workspace_bytes() */
int lisec_detection_iou_loss_weighted(const lisec_detection_iou_loss_cfg* cfg, const lisec_sample_weights* sw,
                                      const float* head, const float* y_cls, const float* y_reg, long long M,
                                      float grad_scale, float* dhead, float* loss_out, long long* counts_out,
                                      void* workspace, size_t workspace_bytes, lisec_stream_t stream);
int lisec_detection_iou_loss_weighted_eval(const lisec_detection_iou_loss_cfg* cfg, const lisec_sample_weights* sw,
                                           const float* head, const float* y_cls, const float* y_reg, long long M,
                                           double* acc, void* workspace, size_t workspace_bytes, lisec_stream_t stream);
size_t lisec_detection_iou_loss_weighted_workspace_bytes(void);    /* = lisec_detection_loss_workspace_bytes() */

/* Metrics that read the label code of the detection loss (csrc/detection_metrics.hip; ours, not Keras').  Inputs and the
 * meaning of pos / neg / ignored as for lisec_detection_loss.  Every metric is a pair {num, den} of sums over the 2M
 * anchors of a sweep; its value is num/den over whatever sweeps the caller pools (0 when den == 0).  With p = sigmoid(z) in
 * double, "predicted" = p > threshold (a NaN logit compares false), t = y_reg - target_offset:
 *   ANCHOR_PRECISION  num #(pos and predicted)                             den #((pos or neg) and predicted)
 *   ANCHOR_RECALL     num #(pos and predicted)                             den N_pos
 *   ANCHOR_ACCURACY   num #(pos and predicted) + #(neg and not predicted)  den N_pos + N_neg
 *   POSITIVE_MAE      num sum_pos sum_k |r_k - t_k|                        den 7 N_pos
 *   POSITIVE_IOU      num sum_pos IoU(decode(r), decode(t))                den N_pos
 * decode is lisec_rpn_decode's arithmetic for the anchor of the channel block, without the anchor centre that both boxes
 * share: centre (r0 l_a, r1 w_a, r2 h_a), extents exp(r3..5) (l_a, w_a, h_a), yaw r6 + yaw_a; IoU is LISEC_IOU_3D /
 * LISEC_IOU_BEV of lisec_boxes_match (below).  A positive whose decoded offsets or extents are not all finite (exp
 * overflows beyond r = 709), or whose IoU is not finite (a yaw that is not finite), contributes IoU 0 and still counts in
 * den.
 * Every anchor is evaluated in double from the fp32 inputs by one thread; per-workgroup fp64 partials in a fixed
 * partition and one finalize in index order: no atomics, the same bits on every run.  Counts are exact integers held in
 * doubles (pooled counts pass 2^24 within a few hundred sweeps). */
#define LISEC_DET_MAX_METRICS 8
enum {
    LISEC_DET_METRIC_ANCHOR_PRECISION = 0,
    LISEC_DET_METRIC_ANCHOR_RECALL = 1,
    LISEC_DET_METRIC_ANCHOR_ACCURACY = 2,
    LISEC_DET_METRIC_POSITIVE_MAE = 3,
    LISEC_DET_METRIC_POSITIVE_IOU = 4
};
typedef struct lisec_detection_metric {
    int kind;                   /* LISEC_DET_METRIC_* */
    int mode;                   /* POSITIVE_IOU: LISEC_IOU_3D / LISEC_IOU_BEV; 0 otherwise */
    double threshold;           /* the three ANCHOR_* kinds: in the open interval (0, 1) */
} lisec_detection_metric;
typedef struct lisec_detection_metrics_cfg {
    int struct_bytes;           /* sizeof(lisec_detection_metrics_cfg), checked */
    int n_metrics;              /* 1 .. LISEC_DET_MAX_METRICS */
    double target_offset;       /* the VoxelNetLoss's */
    double anchors[2][4];       /* l, w, h, yaw: lisec_rpn_cfg's */
    lisec_detection_metric metric[LISEC_DET_MAX_METRICS];
} lisec_detection_metrics_cfg;

/* out[2*n_metrics] = {num0, den0, num1, den1, ...} (device doubles).  accumulate == 0 stores them (the training step: out
 * is a fixed address), accumulate != 0 adds them (evaluation: out is part of the fp64 accumulator).  Fixed addresses, no
 * host reads, no allocation: the two launches record into a step plan.  LISEC_EINVAL, with nothing enqueued: a NULL
 * pointer, M <= 0, a struct_bytes of another size, n_metrics outside 1..LISEC_DET_MAX_METRICS, an unknown kind or mode, a
 * threshold outside (0, 1), a workspace below lisec_detection_metrics_workspace_bytes(). */
int lisec_detection_metrics(const lisec_detection_metrics_cfg* cfg, const float* head, const float* y_cls,
                            const float* y_reg, long long M, double* out, int accumulate, void* workspace,
                            size_t workspace_bytes, lisec_stream_t stream);
size_t lisec_detection_metrics_workspace_bytes(void);

/* optimizers.SGD(lr=0.01, decay=1e-6, momentum=0.9, nesterov=True) (:295) on the flat parameter buffer:
 * v <- m*v - lr_t*g;  w <- w + m*v - lr_t*g;  lr_t = lr/(1 + decay*iterations) is computed by the caller. */
int lisec_sgd_nesterov_step(float* theta, const float* grad, float* velocity, long long n, float lr_t,
                            float momentum, lisec_stream_t stream);

/* The same update with the iteration count kept on the DEVICE, so that a HIP graph captured over a whole training
 * step can be replayed (kernel arguments are frozen in a graph): state = long long[2] {iterations, 0} (the second
 * word is scratch and must be 0 between calls); the kernel computes lr_t = (float)(lr / (1 + decay*iterations)) in
 * double, exactly what the host computes for lisec_sgd_nesterov_step, and increments iterations once every
 * workgroup has read it. */
int lisec_sgd_nesterov_step_dev(float* theta, const float* grad, float* velocity, long long n, double lr,
                                double decay, float momentum, long long* state, lisec_stream_t stream);
/* The same update for a PART of the variables, ahead of the rest of the step: state[0] (the iteration count) is read and NOT
 * incremented -- the call that ends the step (lisec_sgd_nesterov_step_dev over the remaining variables) does that.  The
 * RPN + head variables (94 % of them, model_training.py:245-255) have final gradients long before the middle layers and
 * the VFE are differentiated: their update runs on the second stream under the rest of the backward pass. */
int lisec_sgd_nesterov_step_dev_part(float* theta, const float* grad, float* velocity, long long n, double lr, double decay,
                                     float momentum, const long long* state, lisec_stream_t stream);

/* tf.keras 2.4 optimizers beyond the reference's one (csrc/optim.hip), with the device iteration count of
 * lisec_sgd_nesterov_step_dev: state = long long[2] {iterations, 0}, lr_t = (float)(lr / (1 + decay*iterations)) in
 * double.  advance = 1: state[0] is incremented once every workgroup has read it (the call that ends the step);
 * advance = 0: a PART of the variables ahead of the rest of the step, state[0] is read and left alone.  n % 4 == 0.
 *   SGD, momentum == 0 (velocity NULL):  w <- w - lr_t*g
 *   SGD, momentum > 0:                    v <- m*v - lr_t*g, then w <- w + v (nesterov = 0) or w <- w + m*v - lr_t*g (1) */
int lisec_sgd_step_dev(float* theta, const float* grad, float* velocity /* NULL iff momentum == 0 */, long long n,
                       double lr, double decay, float momentum, int nesterov, long long* state, int advance,
                       lisec_stream_t stream);
/* Adam, t = iterations + 1, b1^t and b2^t in fp32, alpha = lr_t*sqrt(1 - b2^t)/(1 - b1^t):
 *   m <- m + (g - m)(1 - b1);  v <- v + (g^2 - v)(1 - b2);  w <- w - alpha*m/(sqrt(v) + epsilon)
 * AMSGrad when vhat is not NULL: vhat <- max(vhat, v), and vhat takes the place of v in the update of w. */
int lisec_adam_step_dev(float* theta, const float* grad, float* m, float* v, float* vhat /* NULL iff !amsgrad */,
                        long long n, double lr, double decay, float beta1, float beta2, float epsilon, long long* state,
                        int advance, lisec_stream_t stream);

/* The other tf.keras 2.4 optimizers (csrc/optim_keras.hip), with the arithmetic of TF's dense kernels, the same state /
 * advance semantics and lr_t = (float)(lr / (1 + decay*iterations)) (Nadam: (float)lr).  Per-step scalars in fp32.
 * LISEC_EINVAL, nothing enqueued: a NULL pointer, a missing or extra slot, n % 4 != 0, rho or a beta outside [0, 1), a
 * negative momentum, epsilon or schedule_decay, or advance not 0/1.
 * RMSprop, c = 1 - rho; mom is NULL iff momentum == 0, mg is NULL iff !centered:
 *   momentum == 0 (eps outside the root):  rms <- rho*rms + c*g^2;  centered: mg <- rho*mg + c*g, den = rms - mg^2
 *                                          (else den = rms);  w <- w - lr_t*g/(sqrt(den) + eps)
 *   momentum > 0 (eps inside the root):    rms <- rms + (g^2 - rms)*c;  centered: mg <- mg + (g - mg)*c,
 *                                          den = rms - mg^2 + eps (else rms + eps);
 *                                          mom <- momentum*mom + lr_t*g/sqrt(den);  w <- w - mom */
int lisec_rmsprop_step_dev(float* theta, const float* grad, float* rms, float* mom /* NULL iff momentum == 0 */,
                           float* mg /* NULL iff !centered */, long long n, double lr, double decay, float rho,
                           float momentum, float epsilon, int centered, long long* state, int advance,
                           lisec_stream_t stream);
/* Adagrad (accumulator starts at initial_accumulator_value):  acc <- acc + g^2;  w <- w - lr_t*g/(sqrt(acc) + eps) */
int lisec_adagrad_step_dev(float* theta, const float* grad, float* accumulator, long long n, double lr, double decay,
                           float epsilon, long long* state, int advance, lisec_stream_t stream);
/* Adadelta, c = 1 - rho:  ag <- ag*rho + g^2*c;  u = sqrt(av + eps)*rsqrt(ag + eps)*g;  w <- w - u*lr_t;
 *                         av <- av*rho + u^2*c   (ag: accum_grad, av: accum_var) */
int lisec_adadelta_step_dev(float* theta, const float* grad, float* accum_grad, float* accum_var, long long n, double lr,
                            double decay, float rho, float epsilon, long long* state, int advance, lisec_stream_t stream);
/* Adamax, t = iterations + 1, b1^t in fp32:  m <- m + (g - m)(1 - b1);  v <- max(b2*v, |g|);
 *                                            w <- w - lr_t/(1 - b1^t) * (m/(v + eps)) */
int lisec_adamax_step_dev(float* theta, const float* grad, float* m, float* v, long long n, double lr, double decay,
                          float beta1, float beta2, float epsilon, long long* state, int advance, lisec_stream_t stream);
/* Nadam, t = iterations + 1, d = schedule_decay; its lr is NOT divided by 1 + decay*iterations:
 *   mu_t = b1*(1 - 0.5*0.96^(d*t)), mu_t1 = b1*(1 - 0.5*0.96^(d*(t + 1))), P = momentum_cache*mu_t, P1 = P*mu_t1
 *   m <- b1*m + (1 - b1)*g;  v <- b2*v + (1 - b2)*g^2
 *   w <- w - lr*((1 - mu_t)*g/(1 - P) + mu_t1*m/(1 - P1)) / (sqrt(v/(1 - b2^t)) + eps)
 * momentum_cache: one float in device memory (1 before the first step).  Every workgroup reads it; the call that ends
 * the step (advance = 1) stores P into it where it advances state[0], so that both calls of a split step compute the
 * same P and the cache moves once per step. */
int lisec_nadam_step_dev(float* theta, const float* grad, float* m, float* v, float* momentum_cache, long long n,
                         double lr, float beta1, float beta2, float epsilon, float schedule_decay, long long* state,
                         int advance, lisec_stream_t stream);

/* Learning-rate schedules (tf.keras 2.4 optimizers.schedules, OptimizerV2._decayed_lr) read by the update kernels from
 * DEVICE memory, like the iteration count: a recorded step keeps replaying correctly, and the host may rewrite the
 * descriptor between steps (lisec_lr_schedule_set, stream-ordered) without recording the step again.  With s = state[0],
 * the iteration count before the update, every workgroup computes once, in double, rounded to float once:
 *     lr_t = (float)(schedule(s) / (1 + decay*s))
 *   CONSTANT           initial                                                         (decay as before: the by-value entries)
 *   EXPONENTIAL        p = s/decay_steps (floored if flag);  initial * decay_rate^p
 *   PIECEWISE          values[i] for the first i with s <= boundaries[i], else values[n_boundaries]
 *   POLYNOMIAL         flag (cycle): decay_steps *= (s == 0 ? 1 : ceil(s/decay_steps)), else s = min(s, decay_steps);
 *                      (initial - end_learning_rate)*(1 - s/decay_steps)^power + end_learning_rate
 *   INVERSE_TIME       p = s/decay_steps (floored if flag);  initial / (1 + decay_rate*p)
 *   COSINE             s = min(s, decay_steps);  initial * ((1 - alpha)*0.5*(1 + cos(pi*s/decay_steps)) + alpha)
 *   COSINE_RESTARTS    f = s/decay_steps (first_decay_steps);  t_mul == 1: i = floor(f), f -= i;  otherwise
 *                      i = floor(log(1 - f*(1 - t_mul))/log(t_mul)), f = (f - (1 - t_mul^i)/(1 - t_mul))/t_mul^i;
 *                      initial * ((1 - alpha)*0.5*m_mul^i*(1 + cos(pi*f)) + alpha)
 * Parameters a kind does not use are ignored. */
#define LISEC_LR_MAX_BOUNDARIES 64
enum {
    LISEC_LR_CONSTANT = 0,
    LISEC_LR_EXPONENTIAL = 1,
    LISEC_LR_PIECEWISE = 2,
    LISEC_LR_POLYNOMIAL = 3,
    LISEC_LR_INVERSE_TIME = 4,
    LISEC_LR_COSINE = 5,
    LISEC_LR_COSINE_RESTARTS = 6
};
typedef struct lisec_lr_schedule {
    int kind;                 /* LISEC_LR_* */
    int flag;                 /* staircase (EXPONENTIAL, INVERSE_TIME) or cycle (POLYNOMIAL) */
    int n_boundaries;         /* PIECEWISE: 1 .. LISEC_LR_MAX_BOUNDARIES */
    int reserved;             /* 0 */
    double initial;           /* initial_learning_rate (CONSTANT: the learning rate) */
    double decay_steps;       /* decay_steps (COSINE_RESTARTS: first_decay_steps); > 0 */
    double decay_rate;
    double end_learning_rate;
    double power;
    double alpha;
    double t_mul;
    double m_mul;
    double decay;             /* the optimizer's legacy `decay`, applied on top */
    double boundaries[LISEC_LR_MAX_BOUNDARIES];
    double values[LISEC_LR_MAX_BOUNDARIES + 1];
} lisec_lr_schedule;

/* Validates *host_desc (a host pointer) and enqueues its copy into dev_desc (device memory, the address the update
 * kernels are given) on `stream`, ordered after every update already enqueued there.  LISEC_EINVAL, nothing enqueued:
 * NULL pointer, unknown kind, decay_steps <= 0 where the kind divides by it, n_boundaries outside
 * 1..LISEC_LR_MAX_BOUNDARIES for PIECEWISE, or a step plan being recorded on this thread (a plan re-issues launches
 * only: the copy would not be part of it). */
int lisec_lr_schedule_set(lisec_lr_schedule* dev_desc, const lisec_lr_schedule* host_desc, lisec_stream_t stream);
/* lr_out[k] = lr_t at s = state[0] + k, k < n (dev pointers; state is read, never advanced): the device function of the
 * update kernels, for tests. */
int lisec_lr_schedule_eval(const lisec_lr_schedule* sched, const long long* state, long long n, float* lr_out,
                           lisec_stream_t stream);
/* lisec_sgd_step_dev / lisec_adam_step_dev with lr_t from the descriptor `sched` (dev) instead of (lr, decay), and the
 * same state / advance semantics.  Given a CONSTANT descriptor they compute the bits of the by-value entries (nesterov
 * = 1: the bits of lisec_sgd_nesterov_step_dev). */
int lisec_sgd_step_sched(float* theta, const float* grad, float* velocity /* NULL iff momentum == 0 */, long long n,
                         const lisec_lr_schedule* sched, float momentum, int nesterov, long long* state, int advance,
                         lisec_stream_t stream);
int lisec_adam_step_sched(float* theta, const float* grad, float* m, float* v, float* vhat /* NULL iff !amsgrad */,
                          long long n, const lisec_lr_schedule* sched, float beta1, float beta2, float epsilon,
                          long long* state, int advance, lisec_stream_t stream);
/* The same for the optimizers of csrc/optim_keras.hip (a CONSTANT descriptor gives the bits of their by-value entries;
 * Nadam's descriptor is built with decay = 0). */
int lisec_rmsprop_step_sched(float* theta, const float* grad, float* rms, float* mom /* NULL iff momentum == 0 */,
                             float* mg /* NULL iff !centered */, long long n, const lisec_lr_schedule* sched, float rho,
                             float momentum, float epsilon, int centered, long long* state, int advance,
                             lisec_stream_t stream);
int lisec_adagrad_step_sched(float* theta, const float* grad, float* accumulator, long long n,
                             const lisec_lr_schedule* sched, float epsilon, long long* state, int advance,
                             lisec_stream_t stream);
int lisec_adadelta_step_sched(float* theta, const float* grad, float* accum_grad, float* accum_var, long long n,
                              const lisec_lr_schedule* sched, float rho, float epsilon, long long* state, int advance,
                              lisec_stream_t stream);
int lisec_adamax_step_sched(float* theta, const float* grad, float* m, float* v, long long n,
                            const lisec_lr_schedule* sched, float beta1, float beta2, float epsilon, long long* state,
                            int advance, lisec_stream_t stream);
int lisec_nadam_step_sched(float* theta, const float* grad, float* m, float* v, float* momentum_cache, long long n,
                           const lisec_lr_schedule* sched, float beta1, float beta2, float epsilon, float schedule_decay,
                           long long* state, int advance, lisec_stream_t stream);

/* THE CHUNK RULES, of every chunk table below (lisec_reg_chunk, lisec_decay_chunk, lisec_lamb_chunk): the host cuts a
 * variable of n floats into ceil(n / LISEC_REG_CHUNK) chunks.
 *   - offset and count are in floats and multiples of 4; offset is relative to the buffer pointers of the call;
 *   - count <= LISEC_REG_CHUNK;
 *   - a chunk never crosses a variable;
 *   - the chunks of a table are ascending in offset;
 *   - the table is device memory and is NOT checked: every [offset, offset + count) must lie inside every buffer the
 *     entry indexes by it. */

/* Weight regularizers (tf.keras 2.4 regularizers.L1L2; csrc/regularize.hip), run in front of an optimizer entry on the
 * same range and stream.  The host cuts each regularised variable into chunks by the chunk rules above, offsets
 * relative to the theta / grad pointers given; as a chunk never crosses a variable, it carries that variable's
 * (l1, l2).
 *   grad[i] <- grad[i] + 2*l2*w + l1*sign(w) in fp32 (c2 = 2.0f*l2, sign(0) = 0) for every element of every chunk
 *   (grad == NULL: the penalty alone); the elements of a (0, 0) chunk and those outside every chunk keep their bits.
 *   P = sum over chunks of l1*sum|w| + l2*sum w^2: fp64 per thread, wave, workgroup and chunk; the per-chunk partials
 *   (the workspace) are added by a second one-workgroup launch in an order fixed by n_chunks alone.  No atomics: grad
 *   and P have the same bits from run to run.
 *   *penalty = P (accumulate == 0) or *penalty += P (accumulate == 1: the second call of a step whose variables are
 *   updated in two parts); then, with loss_total != NULL, *loss_total = (float)((double)*loss_total + *penalty), once.
 * n_chunks == 0 is valid: the penalty is stored as 0 or kept, the fold still happens, only the second launch is made.
 * Fixed addresses, no host reads, no allocation: both launches record into a step plan.  LISEC_EINVAL, nothing
 * enqueued: NULL theta, chunks, penalty or workspace, n_chunks < 0, accumulate not 0/1, a workspace below
 * lisec_regularize_workspace_bytes(n_chunks), theta or grad not 16-byte aligned.
 * flags = LISEC_REG_GRAD_IS_ZERO: the variable's gradient is identically 0 and NO backward pass writes its slot of grad
 * (here: the bias of a convolution that feeds a training-mode BatchNormalization), so the slot still holds what the
 * step before left there; for such a chunk grad[i] <- 2*l2*w + l1*sign(w) is STORED, not added, and grad is not read.
 * Other bits of flags must be 0 and are ignored. */
#define LISEC_REG_CHUNK 4096
#define LISEC_REG_GRAD_IS_ZERO 1
typedef struct lisec_reg_chunk {
    long long offset;
    int count;
    float l1;
    float l2;
    int flags;      /* 0, or LISEC_REG_GRAD_IS_ZERO */
} lisec_reg_chunk;
size_t lisec_regularize_workspace_bytes(int n_chunks);
int lisec_regularize(const float* theta, float* grad /* NULL: penalty only */, const lisec_reg_chunk* chunks /* device */,
                     int n_chunks, double* penalty /* device [1] */, int accumulate, float* loss_total /* NULL, or device */,
                     void* workspace, size_t workspace_bytes, lisec_stream_t stream);

/* x *= s  (gradient averaging after the data-parallel all-reduce) */
int lisec_scale(float* x, long long n, float s, lisec_stream_t stream);

/* Gradient accumulation of a mini-batch (fit(batch_size=B); csrc/grad_accumulate.hip): one pass over n floats of the
 * flat gradient buffer `grad` and a second buffer `acc` of the same layout (the caller offsets both pointers to the
 * start of its range [lo, hi) and passes n = hi - lo).
 *   LISEC_ACC_BEGIN  acc[i] = grad[i]                        grad is only read, scale is ignored (may be NULL)
 *   LISEC_ACC_ADD    acc[i] = acc[i] + grad[i]               grad is only read, scale is ignored (may be NULL)
 *   LISEC_ACC_END    grad[i] = (acc[i] + grad[i]) * *scale   acc is only read; scale: device float[1], read by the kernel
 * THE ARITHMETIC IS A CONTRACT (tests pin it bit for bit): after BEGIN on g1, ADD on g2 .. g(B-1) and END on gB,
 *   grad = ((((g1 + g2) + g3) + ... ) + gB) * s
 * with every add and then the ONE multiply an IEEE fp32 round-to-nearest-even operation of its own: the add is never
 * contracted into the multiply, nothing is reassociated, denormals are kept, the sign of a zero follows IEEE.  Floats
 * outside [0, n) keep their bits, and so does the buffer a form only reads.  No atomics, one thread per element: the
 * same bits from run to run.  The scale is read from the device (not passed by value) so that a recorded step plan
 * serves batches of any size: the host rewrites the float between replays, stream-ordered.
 * Fixed addresses, no host reads, no allocation: the launch records into a step plan.  n == 0 is valid (nothing is
 * enqueued).  LISEC_EINVAL, nothing enqueued: NULL grad or acc, grad == acc, n < 0 or n % 4 != 0, an unknown mode,
 * LISEC_ACC_END without scale, grad or acc not 16-byte aligned, scale not 4-byte aligned. */
#define LISEC_ACC_BEGIN 0
#define LISEC_ACC_ADD 1
#define LISEC_ACC_END 2
int lisec_grad_accumulate(float* grad, float* acc, long long n, int mode, const float* scale /* device [1] */,
                          lisec_stream_t stream);

/* Weight averaging (optimizers.MovingAverage / optimizers.SWA; csrc/weight_average.hip): one pass per optimizer UPDATE
 * over n floats of the flat parameter buffer `theta` (only read) and a second buffer `avg` of the same layout.  The
 * definition is this project's own restatement of tfa.optimizers.MovingAverage / SWA (parity unpinned).
 * s = state[0] + state_bias is the iteration count BEFORE the update, read by the kernel from the device (state: where
 * the update entries keep the count; state_bias 0 when the pass is enqueued in front of the update that advances the
 * count, -1 behind it), w = theta[i] after the update, a = avg[i]:
 *   LISEC_AVG_EMA   decay_s = 0                                   for s < start
 *                           = min(decay, (1 + k) / (10 + k))       with dynamic != 0, k = s - start
 *                           = decay                                otherwise
 *                   c = (float)(1.0 - decay_s), computed in double once per workgroup and rounded once
 *                   c == 1.0f:  a <- w                 a store, not arithmetic (a - (a - w) is not w in fp32)
 *                   otherwise   a <- a - (a - w) * c
 *   LISEC_AVG_SWA   m = max(0, (s - start) / period) (integer division); a snapshot iff s >= start and
 *                   s == start + m*period
 *                   not a snapshot: a keeps its bits (the launch is made, every thread returns: the host does not know s)
 *                   m == 0:     a <- w
 *                   otherwise   a <- (a * (float)m + w) / (float)(m + 1)
 * THE ARITHMETIC IS A CONTRACT (tests pin it bit for bit): each subtraction, multiply, add and divide above is an IEEE
 * fp32 round-to-nearest-even operation of its own, never contracted into an fma, never reassociated, the divide never
 * replaced by a reciprocal multiply; denormals are kept, the sign of a zero follows IEEE.  theta, the floats outside
 * [0, n) and, off a snapshot, avg keep their bits.  No atomics, one thread per element: the same bits from run to run.
 * *desc is a HOST pointer, validated and copied into the launch.  Fixed addresses, no host reads of device memory, no
 * allocation: the launch records into a step plan and replays correctly at every count.  n == 0 is valid (nothing is
 * enqueued).  LISEC_EINVAL, nothing enqueued: NULL theta, avg, desc or state, theta == avg, n < 0 or n % 4 != 0, theta
 * or avg not 16-byte aligned, state not 8-byte aligned, an unknown kind, start < 0, decay outside [0, 1] or NaN (EMA),
 * period < 1 (SWA).  Fields a kind does not use are ignored.
 * lisec_weight_swap: a[i] <-> b[i], bit for bit, for i < n (same argument checks; a == b is refused).
 * lisec_weight_average_eval: for j < k, at s = state[0] + j: EMA c_out[j] = c; SWA m_out[j] = m, or -1 off a snapshot
 * (device pointers; the output of the other kind may be NULL and is not written): the device function of the pass, for
 * tests. */
enum { LISEC_AVG_EMA = 0, LISEC_AVG_SWA = 1 };
typedef struct lisec_weight_average_desc {
    int kind;            /* LISEC_AVG_* */
    int dynamic;         /* EMA: dynamic_decay */
    long long start;     /* EMA: start_step; SWA: start_averaging */
    long long period;    /* SWA: average_period */
    double decay;        /* EMA: average_decay */
} lisec_weight_average_desc;
int lisec_weight_average(const float* theta, float* avg, long long n, const lisec_weight_average_desc* desc /* host, copied */,
                         const long long* state /* device */, long long state_bias, lisec_stream_t stream);
int lisec_weight_swap(float* a, float* b, long long n, lisec_stream_t stream);
int lisec_weight_average_eval(const lisec_weight_average_desc* desc /* host, copied */, const long long* state /* device */,
                              long long k, float* c_out, long long* m_out, lisec_stream_t stream);

/* Decoupled weight decay (optimizers.AdamW / SGDW / extend_with_decoupled_weight_decay; csrc/weight_decay.hip): one
 * streaming pass over the flat parameter buffer `theta`, run IN FRONT of an optimizer entry on the same range and the
 * same stream -- the order of tfa.optimizers.DecoupledWeightDecayExtension, which decays the variable first and then
 * updates the decayed variable.  The host cuts every DECAYED variable into chunks by the chunk rules (above
 * lisec_reg_chunk), offsets relative to the theta pointer given.  Only the decayed variables are in the table: an
 * excluded variable costs no traffic.
 * coeff: a lisec_lr_schedule in DEVICE memory (written by lisec_lr_schedule_set; its `decay` must be 0).  With s =
 * state[0], the iteration count before the update -- read from the device, NEVER advanced, no ticket taken --
 *     wd_t = (float)schedule(s)     in double, once per workgroup, rounded once (the formulas of the table above)
 * As the coefficient is always read from the device, a recorded step plan replays correctly at every count, the host
 * may rewrite the coefficient between steps without recording again, and both parts of a split update (they read the
 * same count) decay with the same wd_t.  As in tfa, wd_t is NOT multiplied by the learning rate.
 * THE ARITHMETIC IS A CONTRACT (tests pin it bit for bit): for every element w of every chunk
 *     p = wd_t * w;   w <- w - p
 * each an IEEE fp32 round-to-nearest-even operation of its own, never contracted into an fma, never rewritten as
 * w*(1 - wd_t); denormals are kept.  wd_t == 0.0f: every thread returns and theta keeps its bits (the sign of a -0
 * included; the launch is made all the same: the host does not know s).  The floats outside every chunk keep their
 * bits.  No atomics, one thread per element: the same bits from run to run.
 * Fixed addresses, no host reads, no allocation: the launch records into a step plan.  n_chunks == 0 is valid (nothing
 * is enqueued).  LISEC_EINVAL, nothing enqueued: NULL theta, chunks, coeff or state, n_chunks < 0, theta not 16-byte
 * aligned, state not 8-byte aligned.
 * lisec_weight_decay_eval: wd_out[j] = wd_t at s = state[0] + j, j < k (device pointers; state is read, never
 * advanced): the device function of the pass, for tests. */
typedef struct lisec_decay_chunk {
    long long offset;
    int count;
    int reserved;   /* 0 */
} lisec_decay_chunk;
int lisec_weight_decay(float* theta, const lisec_decay_chunk* chunks /* device */, int n_chunks,
                       const lisec_lr_schedule* coeff /* device */, const long long* state /* device */,
                       lisec_stream_t stream);
int lisec_weight_decay_eval(const lisec_lr_schedule* coeff /* device */, const long long* state /* device */, long long k,
                            float* wd_out, lisec_stream_t stream);

/* LAMB (optimizers.LAMB; You et al. 2019; csrc/lamb.hip): layer-wise adaptive Adam, this project's own restatement of
 * tfa.optimizers.LAMB (parity unpinned).  The only update entry that is not element-wise: the step of a
 * variable is scaled by its trust ratio r = ||w|| / ||u||, a reduction over the whole variable.
 * The host cuts every trainable variable into chunks by the chunk rules (above lisec_reg_chunk), offsets relative to
 * the theta / grad / m / v pointers given (all four are indexed alike).  chunk.var is the index of the chunk's variable
 * in `vars`, chunk.flags says whether the variable is decayed (LISEC_LAMB_DECAYED) and whether its ratio is used
 * (LISEC_LAMB_ADAPTED; the chunks of one variable carry the same flags); vars[j] gives variable j's first chunk and
 * chunk count, both counted from the start of the TABLE.  `vars` is device memory and NOT checked either: every var
 * must lie inside `vars` and `ratios`.
 * An entry works on chunks [first_chunk, first_chunk + n_chunks) and variables [first_var, first_var + n_vars) of the
 * tables; the chunk range must be exactly the chunks of the variable range (a variable is never split between two
 * calls).  The partials of chunk c live at workspace[2c], the ratio of variable j at ratios[j], whatever the range: the
 * two parts of a split update use slots of their own, and after the step `ratios` holds every variable's r.
 * With it = state[0], t = it + 1, lr_t as for lisec_adam_step_dev / lisec_adam_step_sched:
 * THE ARITHMETIC IS A CONTRACT.  Each line is one IEEE fp32 round-to-nearest-even operation of its own, never
 * contracted into an fma, never reassociated, the divisions never replaced by reciprocal multiplies, sqrtf correctly
 * rounded, denormals kept:
 *     per launch   omb1 = 1 - beta1;  omb2 = 1 - beta2;  c1 = (float)(1.0 - beta1^t), c2 likewise from beta2:
 *                  the power in double by binary exponentiation over the integer t, the difference in double, rounded
 *                  once -- it cancels (1 - 0.999^8 is 0.008), and in fp32 its error would be 1e-5 of u and of r
 *     pass 1       gg = g*g;  ma = beta1*m;  mb = omb1*g;  m <- ma + mb;  va = beta2*v;  vb = omb2*gg;  v <- va + vb
 *     u            mh = m/c1;  vh = v/c2;  q = sqrtf(vh);  d = q + epsilon;  u = mh/d;
 *                  a DECAYED chunk: p = weight_decay_rate*w;  u = u + p
 *     pass 2       step = r*lr_t;  e = step*u;  w <- w - e
 * Pass 1 writes m and v and keeps u in registers; pass 2 forms u again from the stored m, v and the unchanged w by the
 * same operations, hence with the same bits.  Between them, per variable, in fp64:
 *     S_w = sum w*w,  S_u = sum u*u     per thread, then over the workgroup: one pair of partials per chunk; the
 *                                       chunk partials of a variable are added by one wave -- orders W and V of
 *                                       csrc/reduce.h, fixed by the table alone
 *     r = (float)(sqrt(S_w) / sqrt(S_u))   if the variable is ADAPTED and S_w > 0 and S_u > 0, else exactly 1.0f
 * No atomics other than the iteration ticket: theta, m, v and ratios have the same bits from run to run.  grad is only
 * read.  Floats outside every chunk keep their bits in theta, m and v.  advance as for the other entries: 0 leaves the
 * count alone (a part of the variables ahead of the rest of the step), 1 ends the step; with n_chunks == 0 and advance
 * == 1 the count is still advanced.  Three launches (pass 1, ratios, pass 2), fixed addresses, no host reads, no
 * allocation: they record into a step plan.  LISEC_EINVAL, nothing enqueued: a NULL pointer, theta / grad / m / v not
 * 16-byte aligned, workspace / state / chunks not 8-byte aligned, a negative first or count, n_chunks == 0 with
 * n_vars != 0 or the reverse, n_vars > n_chunks, workspace_bytes below lisec_lamb_workspace_bytes(first_chunk +
 * n_chunks, first_var + n_vars), beta1 or beta2 outside [0, 1), a negative epsilon or weight_decay_rate, advance not
 * 0/1.  HBM traffic: 10 floats per element (6 in pass 1, 4 in pass 2) against Adam's 7. */
#define LISEC_LAMB_DECAYED 1
#define LISEC_LAMB_ADAPTED 2
typedef struct lisec_lamb_chunk {
    long long offset;
    int count;
    int var;        /* index into vars / ratios */
    int flags;      /* LISEC_LAMB_DECAYED | LISEC_LAMB_ADAPTED */
    int reserved;   /* 0 */
} lisec_lamb_chunk;
typedef struct lisec_lamb_var {
    int first_chunk;
    int n_chunks;
} lisec_lamb_var;
size_t lisec_lamb_workspace_bytes(int n_chunks, int n_vars);
int lisec_lamb_step_dev(float* theta, const float* grad, float* m, float* v, const lisec_lamb_chunk* chunks /* device */,
                        int first_chunk, int n_chunks, const lisec_lamb_var* vars /* device */, int first_var, int n_vars,
                        float* ratios /* device [>= first_var + n_vars] */, void* workspace, size_t workspace_bytes,
                        double lr, double decay, float weight_decay_rate, float beta1, float beta2, float epsilon,
                        long long* state, int advance, lisec_stream_t stream);
int lisec_lamb_step_sched(float* theta, const float* grad, float* m, float* v, const lisec_lamb_chunk* chunks /* device */,
                          int first_chunk, int n_chunks, const lisec_lamb_var* vars /* device */, int first_var, int n_vars,
                          float* ratios /* device [>= first_var + n_vars] */, void* workspace, size_t workspace_bytes,
                          const lisec_lr_schedule* sched /* device */, float weight_decay_rate, float beta1, float beta2,
                          float epsilon, long long* state, int advance, lisec_stream_t stream);

/* Gradient clipping (optimizers.clip_gradients; csrc/grad_clip.hip): clipvalue, clipnorm and global_clipnorm of tf.keras
 * 2.4 in this project's own restatement (parity unpinned).  Passes over the flat gradient buffer `grad`, run
 * IN FRONT of an optimizer entry on the same stream: behind the penalty pass (Keras' regularization loss sits in the
 * tape, so its gradient is clipped with the rest) and in front of the decoupled weight decay (which acts on the
 * variable).  The table is LAMB's -- lisec_lamb_chunk / lisec_lamb_var above, every trainable variable cut by the chunk
 * rules, offsets relative to `grad`, chunk.var and var.first_chunk counted from the start of the TABLE, flags ignored:
 * a per-variable norm needs exactly a chunk's variable and a variable's chunks, so no new record type is added.
 * `clip` is the threshold c > 0.  An entry works on chunks [first_chunk, first_chunk + n_chunks) and, for the
 * per-variable norm, variables [first_var, first_var + n_vars), which must be exactly the variables of those chunks.
 * The partial of chunk k lives at workspace[k] (a double), the scale of variable j at scales[j], its norm at norms[j],
 * whatever the range: the two parts of a split update use slots of their own.
 * THE ARITHMETIC IS A CONTRACT (tests pin it bit for bit; the file is compiled with contraction off):
 *   lisec_grad_clip_value    for every element of every chunk: g <- c where g > c, g <- -c where g < -c; every other g
 *                            keeps its BITS -- a NaN (both comparisons are false; this is not fminf(fmaxf())), a -0, a
 *                            denormal.  +-inf become +-c.  One launch, 8 bytes of traffic per element.
 *   lisec_grad_clip_norm     three launches ordered by the stream alone:
 *     1. S_k = sum over chunk k of (double)g*(double)g: the product exact, each addition an fp64 operation of its own,
 *        per thread (one workgroup of 256 per chunk, float4 loads, thread t takes float4 t, t + 256, ...), then over
 *        the workgroup in order W of csrc/reduce.h.  4 bytes per element.
 *     2. one wave per variable: S_k of the variable's chunks in order V of csrc/reduce.h: S.   S not finite (an inf or
 *        a NaN in the variable): scale = NaN.   Otherwise n = sqrt(S) and
 *            scale = (float)((double)c / n)  if n > c,  else exactly 1.0f
 *        formed in fp64, rounded once.  scales[j] = scale;  norms[j] = (float)n  (inf or NaN where S is).
 *     3. a workgroup reads its chunk's scale first.  Exactly 1.0f: the chunk is skipped -- no load, no store, the
 *        gradient keeps its bits.  Otherwise g <- g*scale, one fp32 multiply per element (a NaN scale makes the whole
 *        variable NaN, as tf.clip_by_norm does).
 *   lisec_grad_clip_global_norm_partials   launch 1 over a chunk range: the sum of squares may be taken in parts (on
 *        another stream, under the backward pass), each part into its own slots.
 *   lisec_grad_clip_global_norm_finish     one workgroup of 256 adds ALL partials [0, table_chunks): the strided sums
 *        of order T, then order W over the 256 (csrc/reduce.h) -- an order fixed by table_chunks alone.  scales[0] and
 *        norms[0] by the rule of 2.; then launch 3 over
 *        [first_chunk, first_chunk + n_chunks) with scales[0] for every chunk.
 * The pad floats of a variable, up to a multiple of 4, are inside its chunk as in every other table; they hold 0 in
 * grad and add nothing.  No atomics anywhere: grad, scales and norms have the same bits from run to run.  Floats outside
 * every chunk keep their bits.  Fixed addresses, no host reads, no allocation: every launch records into a step plan;
 * the threshold is a kernel argument (a changed threshold is a new recording).  n_chunks == 0 is valid: nothing is
 * enqueued (finish still stores scales[0] and norms[0]).  LISEC_EINVAL, nothing enqueued: a NULL pointer, grad not
 * 16-byte aligned, workspace or chunks not 8-byte aligned, vars / scales / norms not 4-byte aligned, a negative first or
 * count, norm: n_chunks == 0 with n_vars != 0 or the reverse, or n_vars > n_chunks; finish: first_chunk + n_chunks >
 * table_chunks; workspace_bytes below lisec_grad_clip_workspace_bytes(first_chunk + n_chunks) (finish: of table_chunks);
 * a threshold that is not a finite number > 0. */
size_t lisec_grad_clip_workspace_bytes(int n_chunks);
int lisec_grad_clip_value(float* grad, const lisec_lamb_chunk* chunks /* device */, int first_chunk, int n_chunks, float clip,
                          lisec_stream_t stream);
int lisec_grad_clip_norm(float* grad, const lisec_lamb_chunk* chunks /* device */, int first_chunk, int n_chunks,
                         const lisec_lamb_var* vars /* device */, int first_var, int n_vars, float clip,
                         float* scales /* device [>= first_var + n_vars] */, float* norms /* device, likewise */,
                         void* workspace, size_t workspace_bytes, lisec_stream_t stream);
int lisec_grad_clip_global_norm_partials(const float* grad, const lisec_lamb_chunk* chunks /* device */, int first_chunk,
                                         int n_chunks, void* workspace, size_t workspace_bytes, lisec_stream_t stream);
int lisec_grad_clip_global_norm_finish(float* grad, const lisec_lamb_chunk* chunks /* device */, int table_chunks,
                                       int first_chunk, int n_chunks, float clip, float* scales /* device [>= 1] */,
                                       float* norms /* device [>= 1] */, void* workspace, size_t workspace_bytes,
                                       lisec_stream_t stream);

/* BatchNormalization recalibration (LisecNet.recalibrate_batchnorm; csrc/bn_recalibrate.hip): the moving statistics of
 * every BatchNormalization layer are replaced by statistics of the CURRENT variables over K sweeps, as
 * torch.optim.swa_utils.update_bn does with momentum=None.  This project's own restatement (parity
 * unpinned); no finaliser changes.  Every finaliser updates a moving statistic as m <- (float)((double)m*a + batch*(1 - a)),
 * so a training-mode forward over a ZEROED buffer of moving statistics leaves state[i] = fl32(batch_i * coef_i), coef_i =
 * 1 - a of the finaliser that wrote it (lisec_bn_recalibrate_coef), the batch statistic to 2^-24 relative, the Bessel
 * correction of the conv-sink layers applied as training applies it.
 * `state` is the flat fp32 buffer of the moving statistics (device).  `table` is a HOST array of n_entries records, one
 * per BatchNormalization layer, validated and copied into the launch: the layer's moving mean is state[mean_off, mean_off
 * + C), its moving variance state[var_off, var_off + C), offsets in floats.  The ranges of different records must not
 * overlap (not checked) and must lie inside state (not checked).  With j = (sum of C over the records in front) + c the
 * running channel index and N = the sum of C over all records,
 *     acc: double[3 * N], device, three planes:  S1 = acc[j]   S2 = acc[N + j]   Sq = acc[2N + j]
 * lisec_bn_recalibrate_take -- one launch per sweep, behind its training-mode forward.  For every channel, in fp64, each
 * line an IEEE operation of its own (the division correctly rounded, m*m never contracted into the addition):
 *     m = (double)state[mean_off + c] / coef;   v = (double)state[var_off + c] / coef
 *     S1 <- S1 + m;   S2 <- S2 + v;   Sq <- Sq + m*m
 *     state[mean_off + c] <- +0.0f;   state[var_off + c] <- +0.0f         (ready for the next sweep)
 * lisec_bn_recalibrate_finish -- once, behind the last take (acc is only read):
 *     k = (double)sweeps;   mean = S1/k
 *     LISEC_BN_STATS_MEAN    var = S2/k                                   (update_bn's rule: the mean of the batch variances)
 *     LISEC_BN_STATS_POOLED  var = (S2/k + Sq/k) - mean*mean;  var < 0: var = 0     (plus the variance of the sweeps' means:
 *                            "precise BN"; every sweep weighs the same, whatever its row count)
 *     state[mean_off + c] <- (float)mean;   state[var_off + c] <- (float)var          each rounded once
 * Denormals are kept (fp32 inputs and fp64 arithmetic).  No atomics, every channel owned by one thread, grid-stride
 * loops: the same bits from run to run.  The floats of state outside every record -- the alignment pads -- are never read
 * or written.  Fixed addresses, no host reads of device memory, no allocation.
 * LISEC_EINVAL, nothing enqueued: NULL state, table or acc; n_entries < 1 or > LISEC_BN_RECAL_MAX_ENTRIES; a record with C
 * < 1, coef outside the open interval (0, 1) (or NaN), a negative offset or one that is not a multiple of 4 floats;
 * state not 4-byte or acc not 8-byte aligned; finish: sweeps < 1, an unknown `statistics`.
 * lisec_bn_recalibrate_coef: coef of a finaliser family (host; 0.0 for an unknown family):
 *     LISEC_BN_FINALIZER_CONV  1.0 - 0.99            lisec_bn_finalize (bn.hip) and the in-kernel finaliser of a lisec_bn_sink
 *     LISEC_BN_FINALIZER_VFE   1.0 - (double)0.99f   the VFE finaliser (vfe.hip); 9.5e-7 relative away from the other */
#define LISEC_BN_RECAL_MAX_ENTRIES 64
enum { LISEC_BN_STATS_MEAN = 0, LISEC_BN_STATS_POOLED = 1 };
enum { LISEC_BN_FINALIZER_CONV = 0, LISEC_BN_FINALIZER_VFE = 1 };
typedef struct lisec_bn_recal_entry {
    long long mean_off;  /* floats into state; a multiple of 4 */
    long long var_off;   /* likewise */
    int C;               /* channels */
    int reserved;        /* 0 */
    double coef;         /* 1 - momentum of the layer's finaliser: lisec_bn_recalibrate_coef */
} lisec_bn_recal_entry;
double lisec_bn_recalibrate_coef(int family);
int lisec_bn_recalibrate_take(float* state, const lisec_bn_recal_entry* table /* host, copied */, int n_entries,
                              double* acc /* device [3 * sum C] */, lisec_stream_t stream);
int lisec_bn_recalibrate_finish(float* state, const lisec_bn_recal_entry* table /* host, copied */, int n_entries,
                                const double* acc /* device [3 * sum C] */, long long sweeps, int statistics,
                                lisec_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * 4b. Data-parallel gradient exchange.  The reference trains in ONE process
 *     (model.fit, model_training.py:299); here whole samples are sharded over one process per GPU and the
 *     only exchange of a step is the all-reduce of the flat gradient buffer, followed by identical
 *     lisec_sgd_nesterov_step calls on every rank.
 *     lisec_comm_t is an RCCL communicator (ncclComm_t): make one with lisec_comm_unique_id (one rank;
 *     ship the LISEC_COMM_ID_BYTES to the others by any means) + lisec_comm_init (every rank, after
 *     hipSetDevice), or pass a communicator the caller already owns.  RCCL is resolved at run time from the
 *     copy the process has loaded (librccl.so.1).
 *     lisec_allreduce_grads: grad[0..n) <- sum over ranks / world, in place, enqueued on `stream` (RCCL
 *     all-reduce + the scale kernel).  `world` is the divisor (the communicator's size for a mean).  Call it
 *     on sub-ranges of the buffer to overlap the exchange with the rest of the backward pass: the RPN + head
 *     gradients -- the tail of the buffer, 94 % of it -- are final long before the middle/VFE ones.
 * ------------------------------------------------------------------------------------------ */
#define LISEC_COMM_ID_BYTES 128
typedef void* lisec_comm_t; /* ncclComm_t */
int lisec_comm_unique_id(void* id /* LISEC_COMM_ID_BYTES, host */);
int lisec_comm_init(int rank, int world, const void* id, lisec_comm_t* comm);
int lisec_comm_destroy(lisec_comm_t comm);
/* LISEC_OK when RCCL can be loaded in this process.  No collective, no device work: every rank calls it BEFORE the
 * collective lisec_comm_init, so that a rank without RCCL is found while the others can still be told. */
int lisec_comm_probe(void);
/* Number of ranks of the communicator (ncclCommCount). */
int lisec_comm_count(lisec_comm_t comm, int* count);
/* world: 0 = divide by the communicator's own size; > 0 must EQUAL it (a mismatch would mis-scale every gradient and is
 * refused with LISEC_EINVAL); < 0 = an explicit divisor -world. */
int lisec_allreduce_grads(lisec_comm_t comm, float* grad, long long n, int world, lisec_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * 5. Box geometry either side of the network; float64 like the reference.
 *    Anchor grid of rpnToRegion.py:75-150 / serialize_data.py:201-232: outX x outY cells of vx x vy metres
 *    (nx/2, ny/2, 2*voxelx, 2*voxely), two anchors (l, w, h, yaw) per cell.
 * ------------------------------------------------------------------------------------------ */
typedef struct {
    int outX, outY;
    double vx, vy;
    double anchors[2][4];
} lisec_rpn_cfg;

/* rpnToRegion (rpnToRegion.py:113-164): decode cls (outX*outY rows of cls_stride floats, 2 used) and reg
 * (rows of reg_stride floats, 14 used) into boxes, then greedy NMS (nonMaxSuppressionFast, :18-72) with the
 * rotated IoU of serialize_data.py:138-178.  The reference calls it with maxBoxes=20, overlapThresh=0.
 * out_boxes: double[(max_boxes+1)*7], out_probs: double[max_boxes+1], out_count: device int32. */
size_t lisec_rpn_to_region_workspace_bytes(const lisec_rpn_cfg* cfg, int max_boxes);
int lisec_rpn_to_region(const lisec_rpn_cfg* cfg, const float* cls, int cls_stride, const float* reg,
                        int reg_stride, double overlap_thresh, int max_boxes, void* workspace,
                        size_t workspace_bytes, double* out_boxes, double* out_probs, int32_t* out_count,
                        lisec_stream_t stream);

/* The decode alone (rpnToRegion.py:118-158: anchor grid + applyRegrssion, rows anchor-major as the reference's reshape at
 * :146-148): boxes double[2*outX*outY*7], probs double[2*outX*outY], legal int32[2*outX*outY] (0 where :155-158 removes
 * the box).  What lisec_rpn_to_region runs first; exposed so that it can be checked against the reference's own decode. */
int lisec_rpn_decode(const lisec_rpn_cfg* cfg, const float* cls, int cls_stride, const float* reg, int reg_stride,
                     double* boxes, double* probs, int32_t* legal, lisec_stream_t stream);
/* The box geometry the kernels use, for parity checks: corners double[n*4*2] = boxToShapely's [topRight, botRight, botLeft,
 * topLeft] (serialize_data.py:149-162) of boxes double[n*7]; per pair (2k, 2k+1): pair_out double[(n/2)*4] =
 * {calculateIntersection volume (:140-147), calculateUnion (:165-168), IoU (:178), this library's own polygon area},
 * the first three with the polygon area TAKEN from pair_area[k] when it is not NULL (the reference delegates that area to
 * shapely). */
int lisec_box_geometry(const double* boxes, int n, const double* pair_area, double* corners, double* pair_out,
                       lisec_stream_t stream);

/* preprocessLabels up to the class/regress maps before balancing (serialize_data.py:194-307).
 * fixed_boxes: device double[n_boxes*7], ALREADY scaled by fixBoxScaling (:181-191).
 * valid/overlap: double[outX*outY*2], out_regress: double[outX*outY*14] (all overwritten), indexed with the
 * reference's wrap-around of negative voxel indices. */
size_t lisec_rpn_labels_workspace_bytes(int n_boxes);
int lisec_rpn_labels(const lisec_rpn_cfg* cfg, const double* fixed_boxes, int n_boxes, double iou_lo, double iou_hi,
                     void* workspace, size_t workspace_bytes, double* valid, double* overlap, double* out_regress,
                     lisec_stream_t stream);

/* calcIntersectAll / calcUnionAll (rpnToRegion.py:202-222), the score of rpnToRegion.py:253-255, for n_samples samples in
 * one launch.  Sample s owns rows pred_start[s] .. pred_start[s+1] of pred_boxes and label_start[s] .. label_start[s+1]
 * of label_boxes (device int32[n_samples+1], device double[rows*7]); a footprint is boxToShapely's quadrilateral
 * (serialize_data.py:151-163) in whatever orientation it comes, a box with l == 0 or w == 0 has none.
 * out: device double[n_samples*5] = {area((U pred) n (U label)) (the reference's cascaded_union(...).intersection(...).area,
 * :207-213), area(U pred), area(U label), sum of pred l*w*h, sum of label l*w*h (predictSum, annsSum of :216-221)}.
 * Exact float64 geometry (a boundary integral over the rectangle edges), summed in a fixed order: bit-identical from run
 * to run.  The workspace is not needed today (0 bytes; NULL is accepted). */
size_t lisec_boxes_union_overlap_workspace_bytes(int n_samples, int max_pred, int max_label);
int lisec_boxes_union_overlap(const double* pred_boxes, const int32_t* pred_start, const double* label_boxes,
                              const int32_t* label_start, int n_samples, void* workspace, size_t workspace_bytes,
                              double* out, lisec_stream_t stream);

/* Detection average precision: score-ranked boxes against annotations at IoU thresholds (csrc/detection_ap.hip).  Not in the
 * reference; the rule is the PASCAL-VOC style one of DESIGN section 7, parity with the Lyft devkit unpinned.
 *
 * lisec_boxes_match: the samples are laid out as for lisec_boxes_union_overlap, with pred_start[0] == 0; total_pred =
 * pred_start[n_samples] and total_pairs = sum over the samples of n_pred * n_label are the sizes the HOST sized the buffers
 * by.  IoU of a prediction p and a label g, footprints as above (a negative extent mirrors one):
 *   LISEC_IOU_3D   inter = area(fp_p n fp_g) * max(0, min(z_p + |h_p|/2, z_g + |h_g|/2) - max(z_p - |h_p|/2, z_g - |h_g|/2)),
 *                  union = |l w h|_p + |l w h|_g - inter, iou = inter / union, 0 when union <= 0 -- geometrically consistent,
 *                  NOT calculateIoU (serialize_data.py:170-178) with its unclamped z term;
 *   LISEC_IOU_BEV  the same with areas only;
 *   a box with l == 0 or w == 0 (or h == 0 under LISEC_IOU_3D) has IoU 0 with everything.
 * Per prediction: best_label = the row, within its own sample, of the label with the largest IoU (the lowest row among
 * equals; -1 without labels), best_iou = that IoU.  Per threshold t (HOST double[n_thresholds], 1..16 values in [0, 1)), in
 * the order of descending score, equal scores by ascending row: a prediction is a true positive when best_iou > t and no
 * earlier one has taken best_label at t, and then takes it; tp: uint8[n_thresholds][total_pred] in input order, tp_count:
 * int32[n_samples][n_thresholds].  On return the first total_pairs doubles of the workspace hold the IoU matrices, sample
 * after sample, each n_pred x n_label row-major.  No size is capped: the pair kernel strides over total_pairs with a bounded
 * grid, and the workspace the caller can supply is the only limit.  Offsets that disagree with total_pred / total_pairs give
 * best_iou = NaN, best_label = -1, tp = 0, tp_count = -1 (and NaN matrices).  Integers and float64 in a fixed order:
 * bit-identical from run to run.
 *
 * lisec_boxes_pair_iou: the IoU matrices alone, in the same layout, into out_iou (device double[total_pairs]); NaN throughout
 * when the offsets disagree with the sizes.  workspace: lisec_boxes_match_workspace_bytes(n_samples, total_pred, 0, 1) bytes.
 *
 * lisec_boxes_average_precision: rank[k] = the row of the prediction ranked k-th (device int64[n_pred], e.g. a stable
 * descending sort of the scores), tp as above, n_labels = G > 0 (LISEC_EINVAL for G <= 0).  With cum_k the true positives
 * among the first k ranks: rec_k = cum_k / G, prec_k = cum_k / k, mrec = [0, rec.., 1], mpre = [0, prec.., 0] made
 * non-increasing from the right, out_ap[t] = sum (mrec[i+1] - mrec[i]) * mpre[i+1]; 0 for n_pred == 0.  out_curve, when not
 * NULL: double[n_thresholds][n_pred][2] = (rec_k, prec_k before the envelope).  One workgroup per threshold. */
#define LISEC_IOU_3D 0
#define LISEC_IOU_BEV 1
size_t lisec_boxes_match_workspace_bytes(int n_samples, int total_pred, long long total_pairs, int n_thresholds);
int lisec_boxes_match(const double* pred_boxes, const double* pred_scores, const int32_t* pred_start,
                      const double* label_boxes, const int32_t* label_start, int n_samples, int total_pred,
                      long long total_pairs, const double* thresholds, int n_thresholds, int mode, void* workspace,
                      size_t workspace_bytes, double* best_iou, int32_t* best_label, uint8_t* tp, int32_t* tp_count,
                      lisec_stream_t stream);
int lisec_boxes_pair_iou(const double* pred_boxes, const int32_t* pred_start, const double* label_boxes,
                         const int32_t* label_start, int n_samples, int total_pred, long long total_pairs, int mode,
                         void* workspace, size_t workspace_bytes, double* out_iou, lisec_stream_t stream);
int lisec_boxes_average_precision(const int64_t* rank, const uint8_t* tp, int n_pred, int n_labels, int n_thresholds,
                                  double* out_ap, double* out_curve, lisec_stream_t stream);

/* Detection evaluation (csrc/detection_eval.hip): the matcher and integrator above with ignored labels and predictions, a
 * heading-aware score, the true-positive errors and the best-F1 operating point.  Not in the reference; DESIGN section 7.
 * The entries above keep their results bit for bit; without flags, best_iou, best_label, tp_count, state == tp and the AP
 * word here equal theirs bit for bit.  An addition changes no signature: the ABI version stays.
 *
 * lisec_boxes_evaluate: layout, sizes, IoU, thresholds, mode and the consistency word are lisec_boxes_match's.  pred_ignore:
 * device uint8[total_pred] or NULL, label_ignore: device uint8[total_labels] or NULL (NULL: no flag set); non-zero = ignored.
 *   Candidate.  best_label[i] = the row, within the prediction's own sample, of the NON-ignored label with the largest IoU
 *     (the lowest row among equals; -1 when the sample has none), best_iou[i] = that IoU (0 without one); ignored_iou[i] =
 *     the largest IoU with an ignored label of its sample (0 without one).
 *   State at threshold t, in the order of descending score, equal scores by ascending flat row:
 *     1 (TP) when best_iou > t and no earlier-ranked prediction of the sample with the same candidate has best_iou > t;
 *     else 2 (ignored) when ignored_iou > t or pred_ignore[i]; else 0 (FP).
 *     An ignored label absorbs any number of predictions; a prediction with pred_ignore set can still be a TP and then takes
 *     its label.  state: uint8[n_thresholds][total_pred] in input order, tp_count: int32[n_samples][n_thresholds] (the 1s).
 *   geom[i] = (sim, dist, scale, yaw) against the candidate, all NaN when best_label == -1 (double[total_pred][4]):
 *     sim = (1 + cos(yaw_p - yaw_g)) / 2;  dist = sqrt(dx^2 + dy^2) of the centres;
 *     scale = 1 - v / (V_p + V_g - v) with V = |l w h| and v = min|l| * min|w| * min|h| (one minus the IoU of the two boxes
 *     made concentric and parallel; 1 when the denominator is <= 0);  yaw = |atan2(sin d, cos d)| in [0, pi], d = yaw_p - yaw_g.
 *   Offsets that disagree with total_pred / total_pairs give best_iou = NaN, best_label = -1, state = 0, tp_count = -1 (and
 *   NaN ignored_iou, geom and IoU matrices).  workspace: lisec_boxes_evaluate_workspace_bytes bytes (0 for sizes it refuses);
 *   on return its first total_pairs doubles hold the IoU matrices.
 *   LISEC_EINVAL, nothing launched: a NULL output, 0 or more than 16 thresholds, a threshold outside [0, 1), an unknown mode,
 *   too small a workspace, a buffer misaligned for its element type.
 *
 * lisec_boxes_evaluate_integrate: rank as for lisec_boxes_average_precision, state / geom / scores as above (scores =
 * pred_scores), n_labels = G = the number of NON-ignored labels (> 0, else LISEC_EINVAL).  Ignored ranks (state 2) are
 * skipped.  With cumTP, cumFP and cumSim (the sum of sim over the TPs) up to rank k: rec = cumTP / G, prec = cumTP / (cumTP
 * + cumFP), os = cumSim / (cumTP + cumFP).  out: double[n_thresholds][LISEC_EVAL_WORDS]:
 *   LISEC_EVAL_AP             the recall-weighted sum of the precision envelope from the right: lisec_boxes_average_precision's
 *                             rule on the sequence with the ignored ranks removed;
 *   LISEC_EVAL_AOS            the same sum with the envelope of os (os <= prec pointwise, so AOS <= AP);
 *   LISEC_EVAL_ATE/ASE/AOE    the means of dist / scale / yaw over the TPs at t, summed in flat-row order by a fixed tree; NaN
 *                             without a TP;
 *   LISEC_EVAL_BEST_F1        the maximum of 2 cumTP / (cumTP + cumFP + G) over the non-ignored ranks (0 without one);
 *   LISEC_EVAL_BEST_F1_SCORE  the score of the lowest rank that attains it (NaN without a TP): the score_threshold to hand
 *                             to lisec_detect for that operating point.
 * out_curve, when not NULL: double[n_thresholds][n_pred][3] = (rec, prec, os) per rank before the envelopes, NaN at ignored
 * ranks.  One workgroup per threshold; float64 and integers in a fixed order: bit-identical from run to run. */
#define LISEC_EVAL_WORDS 7
#define LISEC_EVAL_AP 0
#define LISEC_EVAL_AOS 1
#define LISEC_EVAL_ATE 2
#define LISEC_EVAL_ASE 3
#define LISEC_EVAL_AOE 4
#define LISEC_EVAL_BEST_F1 5
#define LISEC_EVAL_BEST_F1_SCORE 6
size_t lisec_boxes_evaluate_workspace_bytes(int n_samples, int total_pred, long long total_pairs, int n_thresholds);
int lisec_boxes_evaluate(const double* pred_boxes, const double* pred_scores, const int32_t* pred_start,
                         const uint8_t* pred_ignore, const double* label_boxes, const int32_t* label_start,
                         const uint8_t* label_ignore, int n_samples, int total_pred, long long total_pairs,
                         const double* thresholds, int n_thresholds, int mode, void* workspace, size_t workspace_bytes,
                         double* best_iou, int32_t* best_label, double* ignored_iou, double* geom, uint8_t* state,
                         int32_t* tp_count, lisec_stream_t stream);
int lisec_boxes_evaluate_integrate(const int64_t* rank, const uint8_t* state, const double* geom, const double* scores,
                                   int n_pred, int n_labels, int n_thresholds, double* out, double* out_curve,
                                   lisec_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * 5b. Many-box detection output (csrc/detect.hip): score cut, exact top-N, greedy rotated NMS over those N, capped.
 *     Not in the reference, whose rpnToRegion loop (lisec_rpn_to_region, section 5) stays what it is; this is the path a
 *     lidar detector's users expect (VoxelNet, SECOND, PointPillars post-processing).  cls, reg, the anchor grid and the
 *     candidate order are lisec_rpn_decode's: candidate i = a * M + m (anchor a, cell m = ix * outY + iy, M = outX * outY)
 *     reads the score cls[m * cls_stride + a] and the seven values reg[m * reg_stride + 7 a ..], and decodes to the row
 *     lisec_rpn_decode writes at i (the same expression; csrc/box_geom.h).
 *
 *  1. Filter and key, one thread per candidate.  A candidate passes when its raw score s (float32) is not NaN and
 *     (double)s > score_threshold, its seven decoded values are finite, its three extents are > 0 and, with inside_only,
 *     0 <= x <= outX * vx and 0 <= y <= outY * vy.  A passing candidate gets the 64-bit key (o(s) << 32) | i, where o maps
 *     the bits u of s to ~u for a set sign bit and to u | 0x80000000 otherwise: unsigned order of o = numeric order of s
 *     (-0.0 below +0.0).  Keys are distinct; equal scores rank the LARGER flat index first (rpnToRegion's tie rule).
 *     A failing candidate gets key 0, which no passing one has.
 *  2. Exact top-N: with P = the number of passing candidates, the L = min(pre_nms_top_n, P) largest keys, found by radix
 *     selection (8-bit digits, integer histograms) and sorted by descending key; rank r = the r-th of them.  Ranks are
 *     decoded to float64 rows; their score is (double)s, or 1 / (1 + exp(-(double)s)) with sigmoid_scores.
 *  3. Suppression matrix: bit b of mask[i][w] is set iff j = 64 w + b satisfies i < j < L and
 *     IoU(box_i, box_j) > iou_threshold, IoU = that of lisec_boxes_match under iou_mode.
 *  4. Greedy reduce in rank order: rank i is kept iff no kept rank before it has bit i set in its row; it stops after
 *     max_boxes kept ranks or at L.  Kept rank number k writes out_boxes[7 k ..], out_scores[k] and out_index[k] = its flat
 *     candidate index i; out_count = {kept, P}.  Nothing past the kept entries is written.
 *  Integers and float64 in a fixed order, no floating-point atomics: bit-identical from run to run.  Four launches on
 *  `stream`, no host synchronisation.  LISEC_EINVAL, nothing enqueued: a NULL pointer, a bad grid, cls_stride < 2,
 *  reg_stride < 14, pre_nms_top_n outside 1..LISEC_DETECT_MAX_TOP_N (one wave64 holds the removed set of the greedy reduce:
 *  64 lanes x 64 bits), max_boxes outside 1..pre_nms_top_n, iou_threshold outside [0, 1) or NaN, a NaN score_threshold, an
 *  iou_mode, sigmoid_scores or inside_only that is none of its values.  LISEC_ENOSPC: workspace_bytes below
 *  lisec_detect_workspace_bytes (0 for arguments that would be refused). */
#define LISEC_DETECT_MAX_TOP_N 4096
typedef struct {
    double score_threshold;  /* compared with the RAW head value: kept iff (double)raw > score_threshold; -INFINITY: none */
    int    sigmoid_scores;   /* 1: out_scores = 1/(1+exp(-raw)) in fp64, 0: raw.  Ranking is always by raw. */
    int    pre_nms_top_n;    /* 1..4096 */
    int    max_boxes;        /* 1..pre_nms_top_n */
    double iou_threshold;    /* [0,1): a candidate is suppressed when IoU with a KEPT higher-ranked box > this */
    int    iou_mode;         /* LISEC_IOU_BEV | LISEC_IOU_3D: pair_iou of csrc/box_geom.h, the IoU the AP uses */
    int    inside_only;      /* 1: drop candidates whose decoded centre lies outside [0,outX*vx] x [0,outY*vy] */
} lisec_detect_cfg;
size_t lisec_detect_workspace_bytes(const lisec_rpn_cfg* cfg, const lisec_detect_cfg* det);
int lisec_detect(const lisec_rpn_cfg* cfg, const lisec_detect_cfg* det, const float* cls, int cls_stride, const float* reg,
                 int reg_stride, void* workspace, size_t workspace_bytes, double* out_boxes /* [max_boxes*7] */,
                 double* out_scores /* [max_boxes] */, int32_t* out_index /* [max_boxes] flat candidate index a*M+m */,
                 int32_t* out_count /* [2]: kept, candidates that passed the filters before the top-N cut */,
                 lisec_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * 5c. Training-time augmentation of a sweep with its boxes (VoxelNet section 3.3) and the label maps of the moved boxes,
 *     on the device (csrc/augment.hip).  Not in the reference, which trains on fixed sweeps and precomputed labels.
 *     Box rows are (x, y, z, l, w, h, yaw) float64 in ego-centred metres as boxes.annotationBoxes returns them; z is the box
 *     CENTRE, the z extent [z - h/2, z + h/2].  The footprint is boxToShapely's (section 5): axes u = (cos yaw, -sin yaw)
 *     with half extent w/2 and v = (sin yaw, cos yaw) with half extent l/2.  A point is inside a box iff |d.u| <= w/2,
 *     |d.v| <= l/2 and z lies in the z extent (all closed); a point inside several boxes belongs to the lowest index.
 *     Random numbers: Philox4x32-10, key = seed (low word, high word), counter = (stream, item, epoch, index), stream 0 =
 *     global, 1 = per box, 2 = balance, 3 = object sampling, 4 = the voxeliser's per-voxel subsample (section 1b); uniform = (u32 + 0.5) * 2^-32 and Box-Muller normals (z0 = r cos t, z1 = r sin t,
 *     r = sqrt(-2 ln u1), t = 2 pi u2), both in double.  Every entry only enqueues on `stream`: no host synchronisation.
 *
 * lisec_augment_draw, one workgroup.  Global: words w = Philox(0, item, epoch, 0): s = scale_lo + (scale_hi - scale_lo) *
 *   u(w0), alpha = rot_global * (2 u(w1) - 1), a counter-clockwise rotation about the z axis through the origin.  Box b, in
 *   index order, attempt a < attempts: w = Philox(1, item, epoch, 2 (b * LISEC_AUG_MAX_ATTEMPTS + a)), w' = the same at
 *   index + 1; dyaw = rot_box * (2 u(w0) - 1), (dx, dy) = sigma[0..1] * BoxMuller(w1, w2), dz = sigma[2] * z0 of
 *   BoxMuller(w'0, w'1).  The first attempt whose footprint (centre + (dx, dy), yaw + dyaw) has intersection area exactly
 *   0 with the CURRENT footprint of every other box (perturbed for lower indices, original for higher ones) is accepted;
 *   with none the box stays put.  Outputs (device): transforms double[n_boxes][4] = (dx, dy, dz, dyaw); global double[2] =
 *   (s, alpha); boxes_out double[n_boxes][7] = the rows after both stages (centre moved, rotated and scaled; l, w, h
 *   scaled; yaw + dyaw - alpha: with these axes a counter-clockwise turn lowers yaw); attempt int32[n_boxes] = the accepted
 *   attempt or -1; draws uint32[4 + 8 n_boxes] = the global words, then per box the eight words (w, w') of the accepted
 *   attempt (0 without one).  A parameter of 0 (attempts 0, scale_lo = scale_hi = 1) makes its stage the identity bit for
 *   bit.  n_boxes > LISEC_AUG_MAX_BOXES or attempts > LISEC_AUG_MAX_ATTEMPTS: LISEC_EINVAL, nothing enqueued.
 *
 * lisec_augment_apply: points (n rows of `stride` elements, 3 used; dtype 0 = float32, 1 = float64) -> points_out (n x 3
 *   dense, same dtype, may not alias), in double: a point inside box b of boxes_before keeps its (d.u, d.v, dz) in the
 *   box's frame while the box takes transforms[b] (an all-zero row leaves its points bit for bit); then every point takes global (rotate, scale x, y and z).  Rows with
 *   |x| >= pad_limit (the pad rows of a recorded step's point buffer) are copied untouched.  The point count is unchanged.
 *
 * lisec_rpn_targets: the label maps of one sweep.  boxes in ego metres; x, l are multiplied by scale_x and y, w by scale_y
 *   (fixBoxScaling, serialize_data.py:181-191) on the device, lisec_rpn_labels sweeps anchors x boxes, and y_cls
 *   float[outX*outY*2] = valid + overlap, y_reg float[outX*outY*14] = out_regress + repeat(overlap, 7) are written at the
 *   caller's addresses.  balance != 0: the balancing of serialize_data.py:310-325 (at most max_regions/2 positives; when
 *   negatives + kept positives exceed max_regions, as many negatives as positives kept) with, instead of random.sample,
 *   the key (Philox(2, item, epoch, flat index)[0] << 32 | flat index) per candidate, flat index = (x * outY + y) * 2 +
 *   anchor: the `keep` smallest keys of a class survive.  balance == 0: float32(preprocessLabels(balance=False)) bit for
 *   bit.
 *
 * Ground-truth object sampling (Yan et al., SECOND, 2018, section 3.2): objects cut out of other training sweeps are pasted
 *   into the current one, collision-checked, BEFORE the noise above is applied.
 *   Database: a flat list of M objects.  Object m is a box row in the ego frame of its source sweep plus the points that box
 *   OWNS under the rule above (closed slab test, lowest box index), in the source sweep's point order and dtype, as absolute
 *   coordinates: db_boxes double[M][7], db_points [P][3], db_offsets int32[M + 1] (object m owns rows db_offsets[m] ..
 *   db_offsets[m + 1]).  Objects are pasted at their original pose (the lidar sampling pattern depends on range and
 *   bearing).  Which objects enter the database (a minimum point count) is the builder's business.
 * lisec_augment_owner: owner int32[n] = the lowest box index holding the point, -1 for none and for pad rows
 *   (|x| >= pad_limit).  What the database is cut out with; the grouping after it is the caller's.
 * lisec_augment_sample, one workgroup.  Philox stream 3: candidate k < n_samples draws w = Philox(3, item, epoch, k) and has
 *   database index (uint64(w0) * M) >> 32 (integer arithmetic).  Candidate k is ACCEPTED iff its footprint has intersection
 *   area exactly 0 with every scene box and with every candidate m < k that was itself accepted: a candidate that collides
 *   only with a rejected earlier one is accepted; the same index drawn twice rejects the second draw by itself; an object
 *   from the item's own sweep collides with its original.  No special cases.  Outputs (device): index int32[n_samples] = the
 *   database index or -1 when rejected; n_boxes_out int32[1] = n_boxes + accepted; boxes_all double[n_boxes + n_samples][7]
 *   = the scene rows, then the accepted rows compacted in order of k, rows past n_boxes_out zero; point_offset
 *   int32[n_samples + 1] = the exclusive prefix of the accepted objects' point counts (a rejected candidate counts 0), the
 *   last entry n_add; draws uint32[4 n_samples] = the words.  M == 0 accepts nothing.  n_samples > LISEC_AUG_MAX_SAMPLES or
 *   n_boxes + n_samples > LISEC_AUG_MAX_BOXES: LISEC_EINVAL, nothing enqueued (refused, not truncated).
 * lisec_augment_paste: points_out has `cap` rows of 3 in the points' dtype (db_points has the same dtype), cap >= n + n_add --
 *   the caller sizes it by the sum of the n_samples largest point counts of the database, which needs no readback; rows past
 *   cap are never written.  Rows [0, n): the scene point (3 of `stride` elements); a live one (|x| < pad_limit) inside an
 *   accepted pasted box (rows n_scene_boxes .. *n_boxes_dev of boxes_all, the closed test) becomes (pad, pad, pad), pad = 2 *
 *   pad_limit; input pad rows are copied untouched.  Rows [n, n + n_add): the accepted objects in order of k, each object's
 *   points in database order, copied bit for bit.  Rows [n + n_add, cap): (pad, pad, pad).  May not alias the input.
 * lisec_augment_draw_n, lisec_augment_apply_n, lisec_rpn_targets_n: the entries above with the box count read from the
 *   device (n_boxes_dev int32[1], what lisec_augment_sample wrote: the number of accepted objects is known only there);
 *   max_boxes >= that count sizes the workspaces and the launch geometry, the kernels bound their loops by min(*n_boxes_dev,
 *   max_boxes).  Rows past the count are neither read nor written.  For equal counts the results equal the host-count
 *   entries' bit for bit.  lisec_rpn_targets_workspace_bytes(cfg, max_boxes) serves both.
 *   The pipeline of one training item: sample, paste into a scratch buffer, draw_n (pasted boxes take the per-box noise too),
 *   apply_n from the scratch into the step's point buffer, rpn_targets_n. */
#define LISEC_AUG_MAX_BOXES 512
#define LISEC_AUG_MAX_ATTEMPTS 32
#define LISEC_AUG_MAX_SAMPLES 64
typedef struct {
    double rot_box;          /* per-box yaw noise: U[-rot_box, rot_box]                     (pi/10) */
    double sigma[3];         /* per-box translation noise: N(0, sigma^2) per axis            (1, 1, 0) */
    double scale_lo, scale_hi; /* global scale: U[scale_lo, scale_hi]                        (0.95, 1.05) */
    double rot_global;       /* global rotation: U[-rot_global, rot_global]                 (pi/4) */
    int attempts;            /* candidates per box                                          (10) */
} lisec_augment_params;
int lisec_augment_draw(const double* boxes, int n_boxes, const lisec_augment_params* params, unsigned long long seed,
                       unsigned int item, unsigned int epoch, double* transforms, double* global, double* boxes_out,
                       int32_t* attempt, uint32_t* draws, lisec_stream_t stream);
int lisec_augment_apply(const void* points, int dtype, int n, int stride, const double* boxes_before, int n_boxes,
                        const double* transforms, const double* global, double pad_limit, void* points_out,
                        lisec_stream_t stream);
size_t lisec_rpn_targets_workspace_bytes(const lisec_rpn_cfg* cfg, int n_boxes);
int lisec_rpn_targets(const lisec_rpn_cfg* cfg, const double* boxes, int n_boxes, double scale_x, double scale_y,
                      double iou_lo, double iou_hi, int balance, int max_regions, unsigned long long seed, unsigned int item,
                      unsigned int epoch, void* workspace, size_t workspace_bytes, float* y_cls, float* y_reg,
                      lisec_stream_t stream);
int lisec_augment_owner(const void* points, int dtype, int n, int stride, const double* boxes, int n_boxes,
                        double pad_limit, int32_t* owner, lisec_stream_t stream);
int lisec_augment_sample(const double* boxes, int n_boxes, const double* db_boxes, const int32_t* db_offsets, int n_objects,
                         int n_samples, unsigned long long seed, unsigned int item, unsigned int epoch, int32_t* index,
                         int32_t* n_boxes_out, double* boxes_all, int32_t* point_offset, uint32_t* draws,
                         lisec_stream_t stream);
int lisec_augment_paste(const void* points, int dtype, int n, int stride, const void* db_points, const int32_t* db_offsets,
                        const int32_t* index, const int32_t* point_offset, const double* boxes_all, int n_scene_boxes,
                        const int32_t* n_boxes_dev, int n_samples, double pad_limit, void* points_out, int cap,
                        lisec_stream_t stream);
int lisec_augment_draw_n(const double* boxes, const int32_t* n_boxes_dev, int max_boxes, const lisec_augment_params* params,
                         unsigned long long seed, unsigned int item, unsigned int epoch, double* transforms, double* global,
                         double* boxes_out, int32_t* attempt, uint32_t* draws, lisec_stream_t stream);
int lisec_augment_apply_n(const void* points, int dtype, int n, int stride, const double* boxes_before,
                          const int32_t* n_boxes_dev, int max_boxes, const double* transforms, const double* global,
                          double pad_limit, void* points_out, lisec_stream_t stream);
int lisec_rpn_targets_n(const lisec_rpn_cfg* cfg, const double* boxes, const int32_t* n_boxes_dev, int max_boxes,
                        double scale_x, double scale_y, double iou_lo, double iou_hi, int balance, int max_regions,
                        unsigned long long seed, unsigned int item, unsigned int epoch, void* workspace,
                        size_t workspace_bytes, float* y_cls, float* y_reg, lisec_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * 5b. Step plans: a whole training step recorded once and re-issued by ONE call (csrc/plan.hip).
 *     The reference repeats one static schedule 180 times (model.fit(batch_size=1, steps_per_epoch=180),
 *     model_training.py:299).  Between lisec_step_plan_begin and lisec_step_plan_end every launch the CALLING THREAD makes
 *     through this library -- on any stream -- and every lisec_event_record / lisec_stream_wait_event is executed as usual
 *     AND appended to the plan with a copy of its arguments; lisec_step_plan_run re-issues them in the recorded order on
 *     the recorded streams (plain launches, no HIP graph).  Arguments are frozen at record time: what changes from step
 *     to step must sit in device memory the recorded launches point at (the sweep in a fixed-capacity point buffer --
 *     pad it with points outside the grid --, the targets, the device-side iteration counter of
 *     lisec_sgd_nesterov_step_dev).  The caller keeps every buffer alive and unchanged in address for the plan's life.
 * ------------------------------------------------------------------------------------------ */
typedef void* lisec_step_plan_t;
int lisec_step_plan_create(lisec_step_plan_t* plan);
int lisec_step_plan_begin(lisec_step_plan_t plan);
int lisec_step_plan_end(lisec_step_plan_t plan);
int lisec_step_plan_run(lisec_step_plan_t plan);
int lisec_step_plan_size(lisec_step_plan_t plan);    /* recorded operations, -1 for NULL */
int lisec_step_plan_recording(void);                  /* 1 while the calling thread records a plan */
int lisec_step_plan_destroy(lisec_step_plan_t plan);
/* hipEventRecord(event, stream) / hipStreamWaitEvent(stream, event, 0) through the library, so that a recording plan sees
 * the fork / join edges between the streams of a step; event: a hipEvent_t the caller made. */
int lisec_event_record(void* event, lisec_stream_t stream);
int lisec_stream_wait_event(lisec_stream_t stream, void* event);
/* A host function as a step of the plan: fn(arg) runs now and, when the calling thread is recording, again at this place of
 * the sequence in every lisec_step_plan_run (0 = success).  For work between a step's launches that is not a launch of
 * this library -- the data-parallel gradient exchange when it goes through torch.distributed (gloo) instead of
 * lisec_allreduce_grads, which records itself. */
int lisec_step_plan_host_call(int (*fn)(void*), void* arg);

/* ------------------------------------------------------------------------------------------
 * 6. Launch-plan tuning and diagnostics.  Not needed by a caller of the hot path: the defaults are the measured
 *    optimum on MI355X; tools/ and bench.py use them to measure the alternatives.
 *    The tuning record is process-wide and read when a call is planned: change it only while no call is in flight.
 * ------------------------------------------------------------------------------------------ */
typedef struct lisec_tuning {
    int struct_bytes;       /* sizeof(lisec_tuning) of the caller (ABI evolution)                              */
    int max_splitk;         /* most K slices per tile                                              (12)        */
    int splitk_min_steps;   /* least 64-deep K steps per slice                                     (3)         */
    int min_splitk;         /* layers that would get fewer slices run unsliced                     (2)         */
    int plane_pair;         /* pair depth planes that run different numbers of taps                (1)         */
    int dense64;            /* resident-workgroup kernel for Dense(64)                             (1)         */
    int half_n;             /* 32-column workgroups instead of two K slices                        (1)         */
    int vfe_shape;          /* launch shape of the VFE stage kernels, -1 = by capacity             (-1)        */
    int field_seg;          /* segment length of the field combine pass, 0 = by capacity           (0)         */
    int field_tpw;          /* taps per workgroup of the field contraction, 0 = by capacity        (0)         */
    int wgrad_blocks;       /* workgroups a weight-gradient launch aims for                        (1024)      */
    int debug_sync;         /* lisec_vfe_backward synchronises and reports after every launch      (0)         */
    int force_splitk;       /* > 0: every sliceable layer gets exactly this many K slices          (0)         */
    int wgrad_combine_max;  /* weight gradients with at most this many slabs per cell sum them in-kernel (32)   */
    int wgrad_batch_blocks; /* workgroups a batched weight-gradient launch aims for                (1024)      */
    int lone_db;            /* small K-sliced layers: one workgroup per CU on the two-image kernels (1)         */
    int wgrad_per_cu;       /* weight-gradient workgroups per CU: 2 leaves 53 KB of LDS for a workgroup of the   */
                            /* data-gradient chain on the other stream (default), 3 = as many as fit            */
    int wgrad_ring;         /* ring kernel for the 3 x 3 stride-1 weight gradients                 (1)         */
    int wgrad_ring_slots;   /* workgroups a ring launch fills, 0 = one per CU                      (0)         */
    int wide_tile;          /* 128 x 128 tiles (512-thread workgroups) for 128-channel w-halo layers of few tiles (0:  */
                            /* measured equal to the 128 x 32 plan alone, 0.8 % slower in the step -- kept for study)   */
    int small_tile;         /* calls that pass LISEC_CONV_SMALL_TILE run small K-sliced layers as 64-row tiles     (1)  */
} lisec_tuning;
int lisec_tuning_get(lisec_tuning* t);        /* fills *t with the current record (t->struct_bytes set)          */
int lisec_tuning_set(const lisec_tuning* t);  /* t->struct_bytes must be sizeof(lisec_tuning); every field is range-checked */
/* STATE OF THE LIBRARY BEYOND ITS ARGUMENTS -- all of it:
 *   1. the tuning record above: ONE per process, unsynchronised; read when a call is PLANNED (so a recorded step plan keeps
 *      the launches it recorded: re-record it after lisec_tuning_set);
 *   2. step-plan recording (5b): per THREAD -- between lisec_step_plan_begin and _end every launch, event edge, host call and
 *      lisec_allreduce_grads of that thread is also appended to the plan;
 *   3. lisec_last_error(): per thread;
 *   4. the lisec_debug_*_stamps pointers: __device__ variables of the code object, NULL unless a diagnostic tool sets them.
 * Everything else -- tensors, workspaces, counters, statistics sinks, communicators, events, streams -- belongs to the caller
 * and is passed in. */
/* Zero-fills a workspace whose head holds arrival counters (the K-sliced contractions of lisec_conv_forward*, every
 * lisec_conv_wgrad*) before its FIRST use; every call leaves those counters at zero again.  Non-zero counters (scratch that
 * was never cleared, a call that was interrupted, two streams sharing one workspace) make slices wait for arrivals that
 * never come: tiles stay unwritten, with no error. */
int lisec_workspace_init(void* workspace, size_t bytes, lisec_stream_t stream);

/* 100 MHz s_memrealtime stamps of thread 0 of every workgroup at the kernels' phase boundaries (tools: igemm_stamps.py, wgrad_stamps.py, vfe_stamps.py, field_stamps.py).
 * buf: device uint64[8192 x 8] (igemm); see the tools for the others; NULL (the default) turns them off -- no stamp
 * instruction executes then.  The pointer is a __device__ variable of the code object: set it from one thread. */
int lisec_debug_igemm_stamps(unsigned long long* buf);
int lisec_debug_wgrad_stamps(unsigned long long* buf);
int lisec_debug_vfe_stamps(unsigned long long* buf);
int lisec_debug_field_stamps(unsigned long long* buf);
int lisec_debug_wino_stamps(unsigned long long* buf);

#ifdef __cplusplus
}
#endif
#endif /* LISEC_HIP_H */
