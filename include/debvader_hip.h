/* debvader_hip.h — C-ABI of libdebvader_hip.so, the MI355X (gfx950) engine behind debvader's
 * create_model_vae / train_* / deblend() call surface.
 *
 * The reference (astrodeepnet/debvader) has no FFI for this path: its boundary is the Python call
 * surface that bottoms out in Keras/TFP (`net.fit`, `net(x)`, `net.compile`, `net.load_weights`).
 * Each entry point below names the reference call it replaces (paths relative to the reference repo).
 * The Python shim in debvader_amd/ binds these with ctypes (see INTEGRATION.md for the stub).
 *
 * Conventions: every call returns an int status (0 = DV_OK, <0 = DV_E_*); dv_last_error() holds the
 * message of the last failure on the calling thread.  Nothing throws or exits across this boundary.
 * The caller owns every host buffer (C-contiguous float32 / int32); the library owns all device memory.
 * A dv_model is not thread-safe.  One process drives one GPU; ranks are joined through RCCL.
 */
#ifndef DEBVADER_HIP_H
#define DEBVADER_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
#if defined(__GNUC__)
#pragma GCC visibility push(default)   /* the library is built with -fvisibility=hidden: these declarations are its surface */
#endif

#define DV_OK 0
#define DV_E_INVALID (-1)
#define DV_E_HIP (-2)
#define DV_E_NOMEM (-3)
#define DV_E_RCCL (-4)
#define DV_E_STATE (-5)
#define DV_E_NODEVICE (-6)

#define DV_MAX_LEVELS 8
#define DV_UNIQUE_ID_BYTES 128

typedef struct dv_ctx dv_ctx;
typedef struct dv_model dv_model;
typedef struct dv_field_set dv_field_set;

/* Architecture + numerics of create_model_vae(input_shape, latent_dim, filters, kernels)
 * (src/debvader/model/model.py:164-218; fixed values used by train_deblender: training/train.py:104-107). */
typedef struct dv_config {
  int32_t height, width, bands;      /* input_shape (59,59,6); square stamps, 1 .. 15 bands (train.py:86 nb_of_bands; the bf16
                                        engine 1 .. 7) */
  int32_t latent_dim;                /* 32; any value 1 .. 64 (model.py:164) */
  int32_t n_levels;                  /* len(filters) */
  int32_t filters[DV_MAX_LEVELS];    /* [32,64,128,256]; multiples of 4 (bf16 engine: of 16) */
  int32_t kernels[DV_MAX_LEVELS];    /* [3,3,3,3]; 1 .. 5 per level (model.py:81-91,121-134), both engines */
  int32_t max_batch;                 /* stamps per device step (workspace capacity) */
  float kl_weight;                   /* KLDivergenceRegularizer weight, model.py:213 (0.01) */
  int32_t kl_multiplicity;           /* times Keras adds the activity loss (2) */
  float bn_eps, bn_momentum;         /* Keras BatchNormalization defaults, model.py:79 (1e-3, 0.99) */
  int32_t bn_moving_var_unbiased;    /* fused-BN moving variance uses the Bessel-corrected batch variance (1) */
  float sigma_floor;                 /* model.py:156 (1e-4) */
  float diag_shift;                  /* model.py:49 (1e-5) */
  int32_t dtype;                     /* DV_DTYPE_F32 (0, the reference's precision) or DV_DTYPE_BF16 (1): bf16 storage and
                                        bf16 MFMA operands for the conv / conv-transpose stacks (model.py:79-98,112-137),
                                        fp32 accumulation, fp32 master weights / Adam / dense trunk / sampler / head */
  int32_t infer_graph;               /* 0 (default) / 1: dv_infer / dv_infer_f64 calls of fewer than 64 stamps in one chunk with
                                        engine-drawn noise replay a captured hipGraph of their forward pass (the ~45 launches of
                                        BASELINE configs[4]'s "hipGraph-captured decode", deblender.py:18) instead of launching
                                        them one by one: first call of a size eager, second captured, then replayed; graphs are
                                        dropped when a parameter changes.  Same bits either way.  Off by default: on MI355X a
                                        one-stamp forward is bound by the duration of its kernels, not by submission */
} dv_config;
#define DV_DTYPE_F32 0
#define DV_DTYPE_BF16 1

/* scalars written by the step functions */
enum { DV_S_LOSS = 0, DV_S_NLL_MEAN = 1, DV_S_KL_REG = 2, DV_S_MSE = 3, DV_N_SCALARS = 4 };

int dv_version(void);
/* 0: the product library (this header is its whole exported surface; it reads no measurement or rehearsal switch);
 * 1: the DEVELOPMENT build (same sources under -DDV_DEBUG_EXPORTS: include/debvader_hip_debug.h, the wrong-result
 * measurement switches DV_EXP_*, the one-GPU rehearsal hook DV_DEBUG_FAKE_PEERS).  The Python package honours its own
 * rehearsal variable (DV_DEBUG_SAME_GPU) only when this returns 1.  No counterpart in the reference (tooling). */
int dv_build_kind(void);
/* CRC-32C of `n` bytes continuing from `crc` (0 to start): the checksum of TensorFlow tensor-bundle checkpoints,
 * which load_weights / ModelCheckpoint read and write (model.py:262-266, train.py:49-75).  Host only. */
uint32_t dv_crc32c(uint32_t crc, const void* data, size_t n);
int dv_last_error(char* buf, size_t n);
int dv_config_default(dv_config* cfg);

/* ---- architecture queries: host only, no GPU needed (replace net.summary(), train.py:118) ---- */
int dv_arch_counts(const dv_config* cfg, int32_t* n_tensors, int64_t* n_encoder, int64_t* n_decoder,
                   int64_t* n_trainable);
int dv_arch_describe(const dv_config* cfg, int32_t i, char* name, size_t name_len, int64_t shape[4], int32_t* ndim,
                     int32_t* trainable);
/* flat layout of the gradient buffer the data-parallel step all-reduces: tensor i occupies
 * [off, off+count) floats; the buckets are, in the order they are reduced, [n_enc_train, n_train) (decoder, queued
 * when the decoder backward is done), [split, n_enc_train) (deep half of the encoder, queued mid-backward) and
 * [0, split) (shallow half, at the end).  out = {split, n_enc_train, n_train, n_total} */
int dv_arch_buckets(const dv_config* cfg, int64_t out[4]);
int dv_arch_offset(const dv_config* cfg, int32_t i, int64_t* off, int64_t* count);
/* forward multiply-accumulates per stamp (padding taps counted), for roofline accounting */
int dv_arch_macs(const dv_config* cfg, int64_t* encoder_macs, int64_t* decoder_macs);

/* ---- context: one per process / GPU -------------------------------------------------------- */
int dv_device_count(int32_t* n);
/* PCI bus id of visible device `device` (>= 16 bytes), without creating a context: the ranks of a job compare
 * (host, bus id) BEFORE they build the communicator, so that two ranks mapped onto one GPU fail fast with a clear message
 * instead of inside ncclCommInitRank (debvader_amd.parallel.make_context).  DV_E_NODEVICE when the index is not visible. */
int dv_device_bus_id(int32_t device, char* bus_id, size_t bus_len);
int dv_comm_unique_id(void* out_id /* DV_UNIQUE_ID_BYTES */);
/* world == 1: id may be NULL.  world > 1: every rank passes rank 0's id (exchanged by the host). */
int dv_ctx_create(int32_t device, int32_t rank, int32_t world, const void* unique_id, dv_ctx** out);
/* Destroys the models still alive on the context first (their handles become invalid), then the communicator, events
 * and streams.  Once the process is inside exit() (the HIP runtime's own exit handlers may have run) both destroy calls
 * only release host memory. */
int dv_ctx_destroy(dv_ctx* ctx);
int dv_ctx_sync(dv_ctx* ctx);
/* sum `n` floats over ranks in place (host buffer); used by the host loop for History scalars */
int dv_ctx_allreduce_host(dv_ctx* ctx, float* buf, int32_t n);

/* What the context's communicator really spans (the multi-rank bench prints it so that a scaling record can be checked):
 * comm_ranks = ncclCommCount (0 without a communicator), comm_rank = this rank inside it, device = HIP device index,
 * bus_id = its PCI bus id (>= 16 bytes), rehearsal = 1 when DV_DEBUG_FAKE_PEERS gave this rank a one-rank communicator
 * although world > 1 (a launch rehearsal on one GPU: nothing is summed across ranks).  Any pointer may be NULL. */
int dv_ctx_comm_info(dv_ctx* ctx, int32_t* comm_ranks, int32_t* comm_rank, int32_t* device, char* bus_id, size_t bus_len,
                     int32_t* rehearsal);
/* Timing of the collectives of the data-parallel step: while enabled, every all-reduce on the comm stream
 * and every wait of the main stream for one is bracketed by timed HIP events.  dv_comm_prof_read synchronises, returns
 * the number of collectives and their summed duration (comm_ms) and the number of main-stream waits and what they cost
 * (exposed_ms: communication NOT hidden behind the backward pass) since the last read, and resets the counters.  The event
 * records perturb the step a little: use a separate pass, not the timed region. */
int dv_comm_prof_enable(dv_ctx* ctx, int32_t on);
int dv_comm_prof_read(dv_ctx* ctx, int64_t* n_collectives, double* comm_ms, int64_t* n_waits, double* exposed_ms);

/* ---- model --------------------------------------------------------------------------------- */
/* replaces create_model_vae (model.py:164); weights start at Keras defaults (Glorot-uniform kernels,
 * zero biases/alphas, BN gamma=1): dv_model_init draws them from the engine's own Philox stream */
int dv_model_create(dv_ctx* ctx, const dv_config* cfg, dv_model** out);
int dv_model_destroy(dv_model* m);
int dv_model_init(dv_model* m, uint64_t seed);
/* tensor i in TF-checkpoint order (dv_arch_describe): replaces net.get_weights / net.load_weights (model.py:266) */
int dv_model_get_param(dv_model* m, int32_t i, float* host, size_t nbytes);
int dv_model_set_param(dv_model* m, int32_t i, const float* host, size_t nbytes);
int dv_model_get_grad(dv_model* m, int32_t i, float* host, size_t nbytes);
/* optimizer slots of tensor i (which = 0: m, 1: v); replaces the checkpoint's .OPTIMIZER_SLOT entries */
int dv_model_get_slot(dv_model* m, int32_t i, int32_t which, float* host, size_t nbytes);
int dv_model_set_slot(dv_model* m, int32_t i, int32_t which, const float* host, size_t nbytes);
/* decoder.trainable = False (train.py:175, model.py:252) takes effect at the next optimizer reset */
int dv_model_set_trainable(dv_model* m, int32_t encoder_trainable, int32_t decoder_trainable);
/* net.compile(optimizer=legacy.Adam(lr)) (train.py:125-130,178-183): fresh slots, iteration 0 */
int dv_optimizer_reset(dv_model* m, float lr, float beta1, float beta2, float eps);
int dv_optimizer_get_iter(dv_model* m, int64_t* iter);
int dv_optimizer_set_iter(dv_model* m, int64_t iter);

/* ---- data resident in HBM (or streamed, below) ----------------------------------------------- */
/* slot 0/1 (train / validation): copies n stamps x[n,H,W,C], y[n,H,W,C] to the device once per fit() */
int dv_data_upload(dv_model* m, int32_t slot, const float* x, const float* y, int64_t n);
int dv_data_free(dv_model* m, int32_t slot);
/* ---- data streamed from host memory (a set larger than HBM) ---------------------------------- */
/* slot 0/1 reads its rows from host memory for every step instead of from HBM.  x, y: n rows of H*W*C elements each
 * contiguous, float32 or float64 (x_f64 / y_f64: cast to float32 as a C cast / numpy's astype do), row_stride_* bytes
 * apart; the caller keeps them alive and unchanged until dv_data_free(slot) or the next dv_data_upload /
 * dv_data_stream_open of the slot.  The step functions then name rows of these arrays; each call gathers its rows
 * into pinned staging and queues their host-to-device copy into a device ring of four batches.  dv_train_steps
 * refuses a streamed slot. */
int dv_data_stream_open(dv_model* m, int32_t slot, const void* x, int32_t x_f64, const void* y, int32_t y_f64,
                        int64_t n, int64_t row_stride_x, int64_t row_stride_y);
/* mode of a slot (0 empty, 1 resident, 2 streamed), its rows, and the bytes it has moved host->device since it was
 * uploaded or opened */
int dv_data_info(dv_model* m, int32_t slot, int32_t* mode, int64_t* n, int64_t* h2d_bytes);
/* free / total device memory of the context's GPU (hipMemGetInfo) */
int dv_ctx_mem_info(dv_ctx* ctx, int64_t* free_bytes, int64_t* total_bytes);

/* ---- steps: replace one Keras train_function / test_function call inside net.fit (train.py:27-37) ---- */
/* Batch = rows idx[0..B) of `slot` (idx == NULL: rows first..first+B).  eps == NULL: the engine draws
 * eps ~ N(0,I) from Philox(seed); else eps[B,latent] is used (parity tests).  global_batch = sum of B over ranks
 * (0: B).  out[DV_N_SCALARS] are the GLOBAL loss, nll mean, kl regulariser and mse (against the predicted mean, or
 * against a sample of the output distribution - Keras' metric - while dv_model_set_mse_sample is on). */
int dv_train_step(dv_model* m, int32_t slot, const int32_t* idx, int64_t first, int32_t B, int32_t global_batch,
                  const float* eps, uint64_t seed, float* out);
/* forward + losses in inference mode (moving BN statistics), no update: Keras validation step */
int dv_eval_step(dv_model* m, int32_t slot, const int32_t* idx, int64_t first, int32_t B, int32_t global_batch,
                 const float* eps, uint64_t seed, float* out);
/* gradients only (training-mode forward + backward, no Adam, no moving-stat update): parity tests */
int dv_grad_step(dv_model* m, int32_t slot, const int32_t* idx, int64_t first, int32_t B, int32_t global_batch,
                 const float* eps, uint64_t seed, float* out);
/* dv_train_step with a deferred result: the step is queued under `ticket` (0..3) and dv_step_result(ticket) later
 * waits for it and returns its scalars, so the host loop of Model.fit (train.py:27-37) can queue the next batch before
 * it reads the previous loss.  The index array is copied before the call returns.  eps is engine-generated. */
int dv_train_step_async(dv_model* m, int32_t slot, const int32_t* idx, int64_t first, int32_t B, int32_t global_batch,
                        uint64_t seed, int32_t ticket);
int dv_step_result(dv_model* m, int32_t ticket, float* out_scalars /* DV_N_SCALARS */);
/* queue K back-to-back training steps on consecutive batches of `slot` without host round trips
 * (bench.py timed region); scalars of the last step are returned */
int dv_train_steps(dv_model* m, int32_t slot, int64_t first, int32_t B, int32_t global_batch, int32_t steps,
                   uint64_t seed, float* out);

/* ---- inference: replaces net(x) in deblend() (deblend_cutout/deblender.py:18,24) ----------- */
/* normalise=True of deblend() (deblender.py:14-22, normalize/normalize.py:3-7): while set, dv_infer / dv_infer_f64 /
 * dv_infer_mc apply tanh(arcsinh(x)) to the staged stamps on the GPU and the inverse, sinh(arctanh(.)), to the
 * predicted mean (the scale stays in normalised units) */
int dv_model_set_normalise(dv_model* m, int32_t on);

/* Keras' "mse" metric of the reference (train.py:128 metrics=["mse", ...]) compares the labels with a SAMPLE of the output
 * distribution (model.py:158 convert_to_tensor_fn = sample), not with its mean.  While set, DV_S_MSE of the step
 * functions is mean((y - (loc + sigma * eps))^2) with eps drawn from the engine's Philox stream (seed of the step, stream
 * 0x4D534500 + rank, counter (stamp, element / 4)); off (default at this level): the squared error against the mean.
 * The Python surface (debvader_amd.model) switches it on when compile(metrics=[..."mse"...]) asks for the Keras metric. */
int dv_model_set_mse_sample(dv_model* m, int32_t on);

/* Gradient / train steps also write the output distribution (loc, scale) of their forward pass, for
 * dv_model_get_activation("loc" / "scale") - what the parity tests compare with the oracle.  Off by default: the
 * train step of the reference (train.py:27) has no reader for them (42 MB of stores per 256-stamp step). */
int dv_model_set_keep_outputs(dv_model* m, int32_t on);
/* x[N,H,W,C] host.  Outputs (any may be NULL): loc/scale [N,H,W,C] = distribution mean / stddev;
 * mu [N,latent], zstd [N,latent] = z.mean()/z.stddev(); z [N,latent] = the sample fed to the decoder. */
int dv_infer(dv_model* m, const float* x, int64_t N, const float* eps, uint64_t seed, float* loc, float* scale,
             float* mu, float* zstd, float* z);
/* same, for float64 stamps (the reference's numpy default): the float32 cast of deblender.py:18 happens while the
 * library stages the array */
int dv_infer_f64(dv_model* m, const double* x, int64_t N, const float* eps, uint64_t seed, float* loc, float* scale,
             float* mu, float* zstd, float* z);
/* deblend() on cutouts of a field without the host round trip: out = net(float32(field[x:x+H, y:y+H, :])) for every
 * start (x, y), H = the network's stamp size.  Replaces the pair extract_cutouts(field, ...) -> deblend(net, cutouts)
 * of DeblendField.deblend_field (deblend/field_deblender.py:260-274 with extract/extraction.py:4-43 and
 * deblend_cutout/deblender.py:18): the float64 field is uploaded once, each chunk's cutouts are gathered and cast on the
 * GPU straight into the network's input buffer, and only mean / stddev travel back.  Results are bit-identical to
 * dv_infer_f64 on the cutouts dv_scene_extract returns (same cast, same kernels, same noise numbering).  Every window
 * must lie inside the field (DV_E_INVALID otherwise); engine-drawn noise only. */
int dv_infer_cutouts(dv_model* m, const double* field, int32_t F, int32_t nb, const int32_t* starts, int64_t N,
                     uint64_t seed, float* loc, float* scale, float* mu, float* zstd, float* z);

/* The same call for a caller that also needs the cutouts themselves: DeblendField.deblend_field's recarray carries
 * `cutout_images` (float64, field_deblender.py:360) and its quality cut compares them with the predicted means (:323-327).
 * `cutouts` [N][H][H][nb] receives field[x:x+H, y:y+H, :] for every start - exact copies of host data, so the library
 * assembles them on the host (the reference's numpy slice assignment, extraction.py:26-32, over the pipeline's copy threads)
 * while the GPU runs the forward passes; they never cross the host link.  loc / scale as in dv_infer_cutouts.  Replaces the
 * reference's sequence extract_cutouts -> deblend (field_deblender.py:260-274) without the float64 D2H -> host cast -> H2D
 * loop that sequence implies on a GPU. */
int dv_infer_cutouts_keep(dv_model* m, const double* field, int32_t F, int32_t nb, const int32_t* starts, int64_t N,
                          uint64_t seed, float* loc, float* scale, double* cutouts);

/* The same, streaming: instead of filling N-stamp result arrays (167 KB per stamp - a million cutouts do not belong on one
 * host) the library hands every finished chunk to `consumer(user, first, count, mean, stddev)`, stamps
 * [first, first + count) in input order, `mean` / `stddev` pointing into the pinned transfer ring (valid until the
 * consumer returns; nothing is copied on the host).  The consumer runs on the calling thread while the GPU works on the
 * next chunks; a non-zero return value stops the call (DV_E_STATE).  Chunks are max_batch stamps (BASELINE configs[4]:
 * 8192). */
typedef int (*dv_chunk_fn)(void* user, int64_t first, int32_t count, const float* mean, const float* stddev);
int dv_infer_cutouts_stream(dv_model* m, const double* field, int32_t F, int32_t nb, const int32_t* starts, int64_t N,
                            uint64_t seed, dv_chunk_fn consumer, void* user);

/* The same forward passes with the consumer that FOLLOWS in the reference fused in, so that no stamp crosses the host link:
 * DeblendField.deblend_field + get_predicted_field + get_residual_field (deblend/field_deblender.py:219-383, :99-189,
 * :46-97) for integer positions.  For every cutout i (window start starts[i], as extract_cutouts computes it) the
 * network's mean and stddev stamps are added on the GPU, in object order, into
 *   mean_field   += stamp placed with its top-left corner at places[i] = (row, col)   (predicted_mean_field)
 *   stddev_field += the stddev stamp at the same place                                  (predicted_stddev_field)
 *   residual_field (optional) = field - the same mean stamps                            (get_residual_field)
 * places[i] is int((F - cs) / 2) + the galaxy's distance to the field centre, as the reference pads and shifts
 * (field_deblender.py:70,130-160); parts of a stamp that leave the field are dropped (scipy.ndimage.shift, mode
 * "constant").  mse_center (optional, [N]) receives each stamp's centre-10x10 MSE against its cutout (:323-327), the input
 * of the reference's quality cut, summed in numpy's pairwise order: the bits of the reference's host formula.  Only the
 * F x F x bands float64 fields (and N doubles) travel back.  Sums are in float64 and in object order: bit-identical to dv_scene_composite on the stamps dv_infer_cutouts returns for the same seed. */
int dv_infer_cutouts_composite(dv_model* m, const double* field, int32_t F, int32_t nb, const int32_t* starts,
                               const int32_t* places, int64_t N, uint64_t seed, double* mean_field, double* stddev_field,
                               double* residual_field, double* mse_center);

/* ---- many fields in one call ----
 * The batched forms of dv_infer_cutouts, _keep and _composite for a survey of many small fields: fields [M][F][F][nb]
 * (float64, host), starts [N][2], and field_ptr [M + 1] (non-decreasing, field_ptr[0] = 0, field_ptr[M] = N): stamps
 * field_ptr[m] .. field_ptr[m + 1] are cut from field m, every window inside its field.  Stamps are numbered 0 .. N-1
 * over all fields; that number is the Philox row of a stamp's noise and the row of its results, and the list runs through
 * the network in the chunks dv_infer makes for N stamps, whatever field a stamp belongs to.  Results are bit-identical to
 * dv_infer_f64 on the concatenated cutouts with the same seed, and each field's composited results to
 * dv_scene_composite on its own stamps in object order: a field never sees another field's stamps.  N < 2^31.
 * The fields are uploaded in groups sized against free device memory (DV_FIELDS_GROUP_MB lowers the group size); a
 * single field that does not fit, or a chunk whose stamps come from more fields than fit, is refused (DV_E_NOMEM).
 * dv_infer_fields_composite: places [N][2] as in dv_infer_cutouts_composite; mean_fields / stddev_fields / optional
 * residual_fields [M][F][F][nb], optional mse_center [N].  A field without stamps gets zeros and residual = field. */
int dv_infer_fields(dv_model* m, const double* fields, int32_t M, int32_t F, int32_t nb, const int32_t* starts,
                    const int64_t* field_ptr, int64_t N, uint64_t seed, float* loc, float* scale, float* mu, float* zstd,
                    float* z);
int dv_infer_fields_keep(dv_model* m, const double* fields, int32_t M, int32_t F, int32_t nb, const int32_t* starts,
                         const int64_t* field_ptr, int64_t N, uint64_t seed, float* loc, float* scale, float* mu,
                         float* zstd, float* z, double* cutouts);
int dv_infer_fields_composite(dv_model* m, const double* fields, int32_t M, int32_t F, int32_t nb, const int32_t* starts,
                              const int32_t* places, const int64_t* field_ptr, int64_t N, uint64_t seed,
                              double* mean_fields, double* stddev_fields, double* residual_fields, double* mse_center);

/* ---- epistemic uncertainty in the many-field calls ----
 * dv_infer_fields_keep and dv_infer_fields_composite with the Monte-Carlo estimate of dv_infer_mc as a stage of the
 * pipeline: behind every chunk's ordinary stochastic pass (`seed`, Philox rows = global stamp numbers, results bit-identical
 * to the calls above) the encoder output that pass left on the GPU is decoded `nsamples` more times (sample k of stamp i
 * draws Philox (mc_seed + k, i)) and folded into per-pixel statistics: no second encoder pass, nothing staged from the host.
 * The std stamps are bit-identical to dv_infer_mc's std_out for the concatenated float32 cutouts, nsamples and mc_seed.
 * _mc_keep: epistemic [N][cs][cs][nb] float32 beside loc, scale and the float64 cutouts (all four required).
 * _mc_composite: epistemic_fields [M][F][F][nb] = the std stamps summed at `places` in float64, object order (the bits of
 * dv_scene_composite on them); eps_norm [N] = sum(std[i,:,:,2]) / sum(mean[i,:,:,2]), both sums float64 (a zero denominator
 * gives IEEE inf / nan); residual_fields and mse_center may be null, the other outputs are required.
 * A resident field costs one more field-sized buffer than in dv_infer_fields_composite.  Refused before any GPU work:
 * nsamples < 1, nb < 3 (the formula reads band 2), a missing output.  The single-field forms are M = 1. */
int dv_infer_fields_mc_keep(dv_model* m, const double* fields, int32_t M, int32_t F, int32_t nb, const int32_t* starts,
                            const int64_t* field_ptr, int64_t N, uint64_t seed, uint64_t mc_seed, int32_t nsamples,
                            float* loc, float* scale, double* cutouts, float* epistemic);
int dv_infer_fields_mc_composite(dv_model* m, const double* fields, int32_t M, int32_t F, int32_t nb, const int32_t* starts,
                                 const int32_t* places, const int64_t* field_ptr, int64_t N, uint64_t seed, uint64_t mc_seed,
                                 int32_t nsamples, double* mean_fields, double* stddev_fields, double* epistemic_fields,
                                 double* residual_fields, double* mse_center, double* eps_norm);

/* ---- sub-pixel positions in the many-field composite call ----
 * dv_infer_fields_composite with the position fit of dv_scene_fit_shifts as a stage of the pipeline and the stamps
 * placed at the fitted positions, all on stamps that stay in device memory.  Behind every chunk's forward pass (`seed`; the
 * network's outputs and mse_center have the bits of the calls above) and, where asked for, its Monte-Carlo stage, the r band
 * (band 2) of the chunk's mean stamps is fitted against the r band of the resident fields - galaxy i from shifts_inout[i]
 * within [-bound, bound]^2, at most max_iter Newton steps, objective / iters / status [N] as dv_scene_fit_shifts returns
 * them and with the bits dv_scene_fit_shifts_fields gives on the stamps dv_infer_fields_keep returns - and the chunk is
 * composited at int((F - cs) / 2) + dist[i] + shifts_inout[i]: an object whose two total positions are integers as an exact
 * translation (the bits of dv_infer_fields_composite), any other with scipy.ndimage.shift's cubic B-spline (order 3, mode
 * "constant") as dv_scene_composite evaluates it, float64 sums in object order.  max_iter = 0 fits nothing: the stamps are
 * placed at the given shifts (objective = J there, status 2).
 * dist [N][2] {row, column}: integer values within +-1e6.  nsamples = 0 with epistemic_fields and eps_norm null: no
 * Monte-Carlo stage; otherwise both are required and filled as by dv_infer_fields_mc_composite (mc_seed, nsamples >= 1).
 * residual_fields and mse_center may be null.  Refused before any GPU work (DV_E_INVALID): nb < 3, a fractional or
 * out-of-range distance, bound outside 0 .. 1e6, max_iter < 0, a non-finite start shift, a missing output.
 * Beside the fields of dv_infer_fields_composite a resident field holds its r-band plane; the fit's workspace (at most
 * 1 GiB) and the B-spline coefficients of 64 stamps are allocated once per call, whatever N is. */
int dv_infer_fields_fit_composite(dv_model* m, const double* fields, int32_t M, int32_t F, int32_t nb, const int32_t* starts,
                                  const double* dist, const int64_t* field_ptr, int64_t N, uint64_t seed, double bound,
                                  int32_t max_iter, double* shifts_inout, uint64_t mc_seed, int32_t nsamples,
                                  double* mean_fields, double* stddev_fields, double* epistemic_fields,
                                  double* residual_fields, double* mse_center, double* eps_norm, double* objective,
                                  int32_t* iters, int32_t* status);

/* Monte-Carlo epistemic uncertainty: encode each stamp once, decode it `nsamples` times with fresh eps, return the
 * mean and the standard deviation (ddof 0) of the predicted means over the samples.  Replaces the per-object loop
 * `np.std(deblend(net, [stamp]*100)[0], axis=0)` of deblend/field_deblender.py:303-313. */
int dv_infer_mc(dv_model* m, const float* x, int64_t N, int32_t nsamples, uint64_t seed, float* mean_out,
                float* std_out);
/* encoder(x) -> t[N, latent + latent(latent+1)/2]  (model.py:61-100) */
int dv_encode(dv_model* m, const float* x, int64_t N, float* t);
/* decoder(z) -> loc, scale  (model.py:103-161) */
int dv_decode(dv_model* m, const float* z, int64_t N, float* loc, float* scale);

/* ---- scene compositing around the network ------------------------------
 * Host buffers are float64 like the reference's numpy arrays; the library stages them through the GPU.
 * dv_scene_extract: out[i] = field[starts[i][0] : +cs, starts[i][1] : +cs, :] for a field [F][F][nb]
 * (extract/extraction.py:4-43; every window must lie inside the field, else DV_E_INVALID).
 * dv_scene_composite: field += sign * sum_i shift(pad(stamps[i]), pos[i]) in object order, where pad() centres the
 * cs x cs stamp in a zero F x F image and shift() is scipy.ndimage.shift with default arguments (order-3 spline,
 * mode "constant"): deblend/field_deblender.py:46-97 (sign -1, the residual field) and :99-189 (sign +1, the
 * predicted mean / stddev / epistemic fields).  pos[i] = {row shift, column shift}. */
int dv_scene_extract(dv_ctx* ctx, const double* field, int32_t F, int32_t nb, const int32_t* starts, int32_t N,
                     int32_t cs, double* out);
int dv_scene_composite(dv_ctx* ctx, double* field, int32_t F, int32_t nb, const double* stamps, const double* pos,
                       int32_t N, int32_t cs, double sign);
/* dv_scene_fit_shifts: the sub-pixel position fit of deblend_cutout/optimization.py (position_optimization), batched.
 * For galaxy i, on the r band only: net = shift(pad(stamps_r[i]), dist[i]), J(s) = mean over the F x F field of
 * (field_r - shift(net, s))^2, minimised over s in [-bound, bound]^2 from shifts_inout[i] (box-projected Newton with
 * analytic derivatives, float64).  field_r [F][F], stamps_r [N][cs][cs], dist / shifts_inout [N][2] as {row, column}.
 * Out: shifts_inout[i] = the fitted shift, objective[i] = J there, iters[i] = accepted Newton steps, status[i] =
 * 0 converged (step or projected gradient below 1e-10 px), 1 converged on a bound, 2 max_iter reached, 3 stalled (no
 * damped step lowered J: the shift is the best one found, not a certified optimum).
 * max_iter = 0 evaluates J at the given shifts and returns status 2.  Distances, start shifts and bound must lie within
 * +-1e6, F within 2 .. 32768; a galaxy whose window needs more than 1 GiB of workspace is refused (DV_E_INVALID).
 * Bit-reproducible for any N. */
int dv_scene_fit_shifts(dv_ctx* ctx, const double* field_r, int32_t F, const double* stamps_r, int32_t N, int32_t cs,
                        const double* dist, double bound, int32_t max_iter, double* shifts_inout, double* objective,
                        int32_t* iters, int32_t* status);
/* dv_scene_fit_shifts for M fields: fields_r [M][F][F], galaxies field_ptr[m] .. field_ptr[m + 1] (field_ptr as in
 * dv_infer_fields) are fitted against field m.  Every galaxy gets what dv_scene_fit_shifts gives it on its own field, bit
 * for bit.  Fields are uploaded in groups sized against free device memory. */
int dv_scene_fit_shifts_fields(dv_ctx* ctx, const double* fields_r, int32_t M, int32_t F, const double* stamps_r,
                               const int64_t* field_ptr, int64_t N, int32_t cs, const double* dist, double bound,
                               int32_t max_iter, double* shifts_inout, double* objective, int32_t* iters, int32_t* status);
/* dv_scene_detect: source detection (reference: detect/detection.py, which runs sep on band 2) on M fields of one band,
 * fields [M][H][W] float64.  SExtractor's method (Bertin & Arnouts 1996) with the rules of DESIGN.md section 7e, float64
 * throughout: sigma-clipped mesh background (exact medians), median-filtered meshes, natural-cubic-spline interpolation,
 * D = correlation of data - back with kernel / sum|kernel|, 8-connected components of D > thresh * globalrms with at least
 * minarea pixels, nthresh-level deblending with contrast cont and the argmax pixel assignment.  Not sep, and not claimed
 * to match it bit for bit.
 * Out: globalrms [M]; offsets [M + 1] (the objects of field f are catalog rows offsets[f] .. offsets[f + 1]); *n_out =
 * the number of objects; the catalog rows field, parent (raster index of the component's first pixel), npix, peak
 * (max D), flux (sum of data - back), x (column) and y (row) barycentres weighted by data - back, ordered by field, then
 * component, then peak pixel.  The rows are written only when *n_out <= cap: call again with cap >= *n_out otherwise
 * (the result is deterministic).  back / rms / D / labels [M][H][W] (each optional, NULL: not returned) are the maps of
 * DESIGN 7e, labels = the component's parent for pixels of kept components, -1 elsewhere.
 * Limits: back_size 1 .. 64, back_filter odd 1 .. 7, kernel odd kh x kw up to 15 x 15 (NULL: the default 7 x 7
 * pixel-integrated Gaussian, sigma 1.27627), H and W up to 2^19 with H * W < 2^31.  Fields are processed in chunks whose
 * device workspace stays under workspace_bytes (0: 4 GiB); a single field that needs more is refused (DV_E_INVALID).
 * Bit-reproducible, and the same for a field whatever the batch it is in. */
typedef struct dv_detect_params {
  double thresh;           /* detection threshold in units of globalrms (1.5) */
  double cont;             /* deblending contrast (1e-5) */
  int32_t minarea;         /* minimum pixels of a component and of a deblending node (4) */
  int32_t nthresh;         /* deblending levels (64) */
  int32_t back_size;       /* background mesh size (64) */
  int32_t back_filter;     /* median filter over the meshes (3) */
  const double* kernel;    /* filter taps [kh][kw] or NULL */
  int32_t kh, kw;
  int64_t workspace_bytes; /* device workspace cap per launch, 0: the default */
} dv_detect_params;
int dv_scene_detect(dv_ctx* ctx, const double* fields, int32_t M, int32_t H, int32_t W, const dv_detect_params* params,
                    int64_t cap, int64_t* n_out, int64_t* offsets, double* globalrms, int32_t* field, int32_t* parent,
                    int32_t* npix, double* peak, double* flux, double* x, double* y, double* back, double* rms,
                    double* D, int32_t* labels);
/* dv_scene_detect_weighted: dv_scene_detect with a per-pixel noise map and a mask.  weights [M][H][W]
 * float64, the convention of the flux fit (7s): a pixel COUNTS iff 0 < w < inf (a comparison: NaN does not count); a data
 * value under a pixel that does not count reaches no sum (selects, never a product with zero), so the fields must be finite
 * only where the pixel counts.  noise = DV_DETECT_NOISE_ABSOLUTE: w is an inverse variance and thresh is in units of the
 * pixel's own sigma; DV_DETECT_NOISE_RELATIVE: w is a relative weight and the threshold is thresh * globalrms (SExtractor's
 * MAP_WEIGHT; with w in {0, 1} a mask only).  The steps of dv_scene_detect with these changes: only counting pixels enter a
 * mesh's clipping; a mesh is good iff 2 * n_counting >= its pixels; a bad mesh takes, for background and rms separately, the
 * mean of the good meshes of its field at the smallest squared mesh distance (ties added in raster order) before the median
 * filter; v = data - back where the pixel counts, 0 elsewhere; the significance map S takes the place of D everywhere
 * downstream (segmentation, deblending levels, core moments, peak; the D map holds S): filter = DV_DETECT_FILTER_CONV:
 * S = (sum kn v) sqrt(w); DV_DETECT_FILTER_MATCHED: S = (sum kn (v w)) / sqrt(sum (kn kn) w), -inf where the denominator is
 * 0; S = -inf at a pixel that does not count.  T = thresh (absolute) or thresh * globalrms (relative).  flux and the
 * barycentres stay sums over v.  A field without a good mesh has no objects, an empty offsets range, globalrms NaN, labels
 * -1 and otherwise unspecified maps; the other fields of the call are untouched.  bad_meshes [M] (nullable): the bad meshes
 * of every field.  With w = 1 everywhere and relative noise, and with w = 1, absolute noise and thresh' = thresh * globalrms,
 * every output has the bits of dv_scene_detect.
 * Refused before any GPU work (DV_E_INVALID, the engine stays usable): what dv_scene_detect refuses, a null struct or null
 * weights, an unknown noise or filter, thresh <= 0 with absolute noise. */
#define DV_DETECT_NOISE_ABSOLUTE 0
#define DV_DETECT_NOISE_RELATIVE 1
#define DV_DETECT_FILTER_CONV 0
#define DV_DETECT_FILTER_MATCHED 1
typedef struct dv_detect_weights {
  const double* weights;   /* [M][H][W] */
  int32_t noise;           /* DV_DETECT_NOISE_* */
  int32_t filter;          /* DV_DETECT_FILTER_* */
} dv_detect_weights;
int dv_scene_detect_weighted(dv_ctx* ctx, const double* fields, int32_t M, int32_t H, int32_t W,
                             const dv_detect_params* params, int64_t cap, int64_t* n_out, int64_t* offsets,
                             double* globalrms, int32_t* field, int32_t* parent, int32_t* npix, double* peak, double* flux,
                             double* x, double* y, double* back, double* rms, double* D, int32_t* labels,
                             const dv_detect_weights* weights, int32_t* bad_meshes);
/* dv_scene_detect_multiband: detection on the inverse-variance weighted combination of k bands.
 * fields [M][H][W][nb] float64, interleaved as the network reads them.  bands->bands: k distinct band numbers, 1 <= k <= nb,
 * their order is the order of every sum; band_weights c_j > 0 finite (NULL: all 1.0), the spectral shape the combination is
 * matched to; planes [M][H][W][k] (NULL: none) with noise as in dv_scene_detect_weighted, one plane per selected band.
 * Per band j the background steps of dv_scene_detect (without planes) or dv_scene_detect_weighted (with P_j) give back_j,
 * rms_j, the band's globalrms g_j and v_j = data_j - back_j.  The band's weight is w_j = 1 / (rms_j rms_j) without planes,
 * P_j / (rms_j rms_j) with relative noise, P_j with absolute noise; band j COUNTS at a pixel iff 0 < w_j < inf, with planes
 * also 0 < P_j < inf, and the band has a good mesh in the field.  Over the counting bands, j ascending:
 * num = sum (c_j w_j) v_j, Wt = sum (c_j c_j) w_j; no counting band: V = Wt = 0 and the pixel does not count; one:
 * V = v_j / c_j; more: V = num / Wt.  Everything behind runs as dv_scene_detect_weighted with (V, Wt) in the place of
 * (v, w), absolute noise and T = thresh (> 0 always: it is in units of the combined pixel's own sigma): D holds the
 * significance S, flux and the barycentres are sums over V.  globalrms[f] = 1 / sqrt(sum (c_j c_j) / (g_j g_j)) over the
 * bands with a good mesh (a diagnostic), NaN for a field without one, which has no objects.  band_globalrms [M][k],
 * bad_meshes [M][k] and the maps back, rms [M][H][W][k], V, Wt, D, labels [M][H][W] are nullable.  With k = 1, c = 1 and no
 * planes every output has the bits of dv_scene_detect_weighted on that band with weights = 1 / (rms rms) of its own maps and
 * absolute noise.
 * Refused before any GPU work (DV_E_INVALID, the engine stays usable): what dv_scene_detect refuses, k < 1 or k > nb, a band
 * out of range or given twice, a c_j that is not finite and positive, an unknown noise or filter, thresh <= 0. */
typedef struct dv_detect_bands {
  const int32_t* bands;        /* [k] */
  int32_t k;
  const double* band_weights;  /* [k] or NULL */
  const double* planes;        /* [M][H][W][k] or NULL */
  int32_t noise;               /* DV_DETECT_NOISE_* (read with planes) */
  int32_t filter;              /* DV_DETECT_FILTER_* */
} dv_detect_bands;
int dv_scene_detect_multiband(dv_ctx* ctx, const double* fields, int32_t M, int32_t H, int32_t W, int32_t nb,
                              const dv_detect_params* params, int64_t cap, int64_t* n_out, int64_t* offsets,
                              double* globalrms, int32_t* field, int32_t* parent, int32_t* npix, double* peak, double* flux,
                              double* x, double* y, double* back, double* rms, double* V, double* Wt, double* D,
                              int32_t* labels, const dv_detect_bands* bands, double* band_globalrms, int32_t* bad_meshes);
/* dv_scene_detect_objects: the detector with the object segmentation map and the isophotal shapes of DESIGN.md section 7zb.
 * nb = 0 with bands = NULL: fields [M][H][W], dv_scene_detect or, with weights, dv_scene_detect_weighted; bands given: fields
 * [M][H][W][nb], dv_scene_detect_multiband (weights must then be NULL).  offsets, globalrms and the seven catalogue arrays
 * have the bits of that call; no back / rms / D / labels come back.  Per object, over the pixels the deblender assigned to
 * it, with D the thresholded map (the significance S in the weighted and multi-band calls) and v the map flux sums (V):
 * the inclusive box xmin xmax ymin ymax; xpeak ypeak, the pixel of peak (max D), and vpeak at xvpeak yvpeak, the largest v,
 * ties to the smallest raster index; dflux = sum D; x_iso, y_iso = sum D c / sum D, sum D r / sum D; x2, y2, xy the second
 * moments about that centre with weights D, to which SExtractor's singular rule is applied (x2 y2 - xy xy < 1/144: x2 and y2
 * gain 1/12); flag: DV_DETECT_FLAG_*.  segmap [M][H][W]: 0 outside every object, k + 1 on the pixels of the object in row
 * offsets[f] + k of field f.  Every pointer of the struct is nullable; the columns [cap] are written like the catalogue,
 * only when *n_out <= cap, the segmap always.
 * Refused before any GPU work (DV_E_INVALID, the engine stays usable): what the corresponding call refuses, a null `objects`,
 * weights together with bands, nb != 0 without bands, thresh < 0 (the weights D must be positive). */
#define DV_DETECT_FLAG_BLENDED 1   /* the object's component gave more than one object */
#define DV_DETECT_FLAG_BORDER 2    /* the box touches the field's border */
#define DV_DETECT_FLAG_SINGULAR 4  /* the singular rule was applied */
#define DV_DETECT_FLAG_MASKED 8    /* weighted / multi-band: a pixel among the 8 neighbours of one of its pixels does not count */
typedef struct dv_detect_objects {
  int32_t *xmin, *xmax, *ymin, *ymax, *xpeak, *ypeak, *xvpeak, *yvpeak, *flag; /* [cap] */
  double *vpeak, *dflux, *x_iso, *y_iso, *x2, *y2, *xy;                        /* [cap] */
  int32_t* segmap;                                                             /* [M][H][W] */
} dv_detect_objects;
int dv_scene_detect_objects(dv_ctx* ctx, const double* fields, int32_t M, int32_t H, int32_t W, int32_t nb,
                            const dv_detect_params* params, int64_t cap, int64_t* n_out, int64_t* offsets, double* globalrms,
                            int32_t* field, int32_t* parent, int32_t* npix, double* peak, double* flux, double* x, double* y,
                            const dv_detect_weights* weights, const dv_detect_bands* bands, const dv_detect_objects* objects);
/* dv_scene_detect_clean: dv_scene_detect_objects followed by the cleaning pass of DESIGN.md section 7zc (after SExtractor's
 * clean.c / sep's clean=True; this project's own rule, not sep's bits).  Over the raw objects of a field, the rows of
 * dv_scene_detect_objects, with T the field's threshold (thresh * globalrms, or thresh in the weighted and multi-band calls),
 * beta = clean_param and pi = 3.141592653589793: det = x2 y2 - xy xy, area = pi sqrt(det), cxx = y2 / det, cyy = x2 / det,
 * cxy = -2 xy / det, a = sqrt((x2 + y2) / 2 + sqrt(((x2 - y2) / 2)^2 + xy^2)), amp = dflux / (2 area),
 * alpha = (pow(amp / T, 1 / beta) - 1) area / npix, and mthresh the minarea-th largest D - T over the object's pixels (0 with
 * fewer).  j is a candidate to absorb i iff j != i, dflux_j > dflux_i (or equal and j < i), T > 0,
 * dx dx + dy dy < 100 (a_i + a_j)^2 with dx = x_iso_i - x_iso_j, dy = y_iso_i - y_iso_j, and P > mthresh_i, where
 * val = 1 + alpha_j ((cxx_j dx) dx + (cyy_j dy) dy + (cxy_j dx) dy) and P = amp_j pow(val, -beta) if 1 < val < 1e10, else 0.
 * absorber[i] is the candidate of the largest P (ties to the smaller row), every object goes to the root of its chain; every
 * test reads the raw values.  The survivors keep their order; a merged row has npix, flux and dflux summed (survivor, then
 * victims in ascending raw row), peak / xpeak / ypeak and vpeak / xvpeak / yvpeak of the member with the largest value (ties
 * to the earlier raw row), the union of the boxes, the OR of the flags with DV_DETECT_FLAG_MERGED, and the survivor's own
 * x, y, x_iso, y_iso, x2, y2, xy and parent.  nmerged: 1 + the victims; mthresh: the survivor's own; n_raw [M]: the raw
 * objects of every field (always written); the segmap carries the cleaned rows' numbers, a victim's pixels its survivor's.
 * A field in which nothing is absorbed keeps the bits of dv_scene_detect_objects in every shared output.  `objects` may be
 * NULL (the catalogue and the clean columns alone); every pointer of `clean` but the struct itself is nullable.
 * Refused before any GPU work (DV_E_INVALID, the engine stays usable): what the underlying call refuses, a null `clean`,
 * clean_param not finite or <= 0, thresh <= 0, minarea > 64. */
#define DV_DETECT_FLAG_MERGED 16   /* the cleaning pass merged other objects into this one */
typedef struct dv_detect_clean {
  double   clean_param;
  int32_t* nmerged;   /* [cap] */
  double*  mthresh;   /* [cap] */
  int64_t* n_raw;     /* [M]   */
} dv_detect_clean;
int dv_scene_detect_clean(dv_ctx* ctx, const double* fields, int32_t M, int32_t H, int32_t W, int32_t nb,
                          const dv_detect_params* params, int64_t cap, int64_t* n_out, int64_t* offsets, double* globalrms,
                          int32_t* field, int32_t* parent, int32_t* npix, double* peak, double* flux, double* x, double* y,
                          const dv_detect_weights* weights, const dv_detect_bands* bands, const dv_detect_objects* objects,
                          const dv_detect_clean* clean);

/* ---- catalogue measurement: fluxes and adaptive moments per galaxy ----
 * The reference ships an empty debvader.measure package; the measurement is defined here, float64 throughout.  Per stamp,
 * with P the network's mean stamp [cs][cs][nb] and S its stddev stamp (float32 widened to double; with normalise on, the
 * denormalised values the composite stage adds), rows r and columns c from 0 to cs - 1:
 *   flux[b] = sum P[r,c,b], flux_err[b] = sqrt(sum S[r,c,b]^2) for every band b;
 *   adaptive moments of I = P[:,:,band]: from r0 = c0 = (cs-1)/2, Mrr = Mcc = sigma0^2, Mrc = 0, iteration k = 1 .. max_iter
 *   weights every pixel of the stamp with w = exp(-(Mcc dr^2 - 2 Mrc dr dc + Mrr dc^2) / (2 det M)) I, dr = r - r0,
 *   dc = c - c0, takes S0 = sum w, mr = sum w dr / S0, mc = sum w dc / S0 and N = 2 (sum w d d^T / S0 - m m^T), then sets
 *   r0 += 2 mr, c0 += 2 mc, M = N.  status 0: 2 max(|mr|,|mc|) < tol and max|N - M| / (Nrr + Ncc) < tol at iteration
 *   iters; 2: max_iter reached (max_iter = 0 returns the initial state); 3: det M not finite or <= 1e-6, S0 not finite or
 *   <= 0 (both before the update of that iteration), or after it a centroid further than cs / 2 from the stamp centre or
 *   a trace Nrr + Ncc that is negative or not finite.  shape[5] = {r0, c0, Mrr, Mrc, Mcc} in their last state whatever
 *   the status.  A stamp's results have the same bits wherever it sits in a batch.
 * dv_scene_measure: host stamps mean / stddev [N][cs][cs][nb] (float32), in chunks sized against free device memory; flux /
 * flux_err [N][nb], shape [N][5], iters / status [N].  stddev and flux_err may be null together.
 * dv_infer_fields_measure: dv_infer_fields_composite with the measurement as one more stage of the pipeline, behind every
 * chunk's forward pass on the chunk's mean and stddev stamps in device memory; the per-stamp outputs are indexed by the
 * global stamp number and have the bits dv_scene_measure gives on the stamps dv_infer_fields returns for the same seed.
 * mean_fields, stddev_fields and residual_fields may be null TOGETHER: the catalogue-only call, in which nothing
 * field-sized is allocated for results or downloaded and places may be null.  With mean_fields and stddev_fields given
 * (residual_fields and mse_center optional) the fields and mse_center have the bits of dv_infer_fields_composite.
 * Refused before any GPU work (DV_E_INVALID) beside what dv_infer_fields_composite refuses: band outside 0 .. nb - 1,
 * sigma0 or tol not finite and positive, max_iter < 0, a missing catalogue output (flux, flux_err, shape, iters, status),
 * mean_fields without stddev_fields or residual_fields without them, a stamp of more than 90 pixels (its float64 band plane
 * does not fit the 64 KB of LDS of a workgroup). */
typedef struct dv_measure_params {
  int32_t band;            /* band of the adaptive moments (2, the r band) */
  double sigma0;           /* initial width in pixels (3.0) */
  double tol;              /* convergence tolerance on the step and on the relative change of M (1e-10) */
  int32_t max_iter;        /* iteration limit (200) */
} dv_measure_params;
int dv_measure_params_default(dv_measure_params* params);
int dv_scene_measure(dv_ctx* ctx, const float* mean, const float* stddev, int64_t N, int32_t cs, int32_t nb,
                     const dv_measure_params* params, double* flux, double* flux_err, double* shape, int32_t* iters,
                     int32_t* status);
int dv_infer_fields_measure(dv_model* m, const double* fields, int32_t M, int32_t F, int32_t nb, const int32_t* starts,
                            const int32_t* places, const int64_t* field_ptr, int64_t N, uint64_t seed,
                            const dv_measure_params* params, double* mean_fields, double* stddev_fields,
                            double* residual_fields, double* mse_center, double* flux, double* flux_err, double* shape,
                            int32_t* iters, int32_t* status);

/* ---- Monte-Carlo catalogue: errors on fluxes and shapes from stochastic decodes ----
 * Sample q of galaxy i is one decoded mean stamp (what dv_infer_mc folds: Philox (mc_seed + q, global stamp number i),
 * denormalised with normalise on).  Every sample is measured as above without a stddev stamp; from its moments follow
 * tr = Mcc + Mrr, det = Mrr Mcc - Mrc^2, sigma = sqrt(sqrt(det)), e1 = (Mcc - Mrr) / tr, e2 = 2 Mrc / tr, and the sample's
 * shape row {row, col, Mrr, Mrc, Mcc, sigma, e1, e2} is accepted iff status == 0, det > 0 and tr > 0 (its flux row always).
 * Per galaxy the rows are folded in ascending sample order with Welford's recurrence (n += 1; d = x - mean; mean += d / n;
 * M2 += d (x - mean); from zeros) and std = sqrt(M2 / n), the population form; every operation is rounded on its own, so a
 * float64 restatement of the same scalar operations gives the same bits.  Outputs, float64: flux_mean / flux_std [N][nb]
 * (n = S), shape_mean / shape_std [N][8] over the n_ok [N] accepted samples (n_ok = 0: NaN; n_ok = 1: std 0).  The
 * per-sample rows sample_flux [N][S][nb], sample_shape [N][S][5], sample_status [N][S] are optional: all given or all null.
 * dv_scene_measure_mc: host sample stamps [S][N][cs][cs][nb] (float32), in chunks of galaxies sized against free device
 * memory.  dv_infer_fields_measure_mc: dv_infer_fields_measure (same arguments, same bits in every output it shares with
 * it) with nsamples more decodes of every chunk's encoder output measured and folded behind its forward pass; the
 * Monte-Carlo catalogue has the bits of dv_scene_measure_mc on the sample stamps dv_infer_mc(nsamples = 1, seed = mc_seed +
 * q) returns for the float32 cutouts.  No epistemic field and no eps_norm are computed.  Refused before any GPU work
 * (DV_E_INVALID) beside what dv_infer_fields_measure refuses: nsamples (S) < 1, a missing Monte-Carlo output, per-sample
 * outputs given in part. */
int dv_scene_measure_mc(dv_ctx* ctx, const float* samples, int32_t S, int64_t N, int32_t cs, int32_t nb,
                        const dv_measure_params* params, double* flux_mean, double* flux_std, double* shape_mean,
                        double* shape_std, int32_t* n_ok, double* sample_flux, double* sample_shape, int32_t* sample_status);
int dv_infer_fields_measure_mc(dv_model* m, const double* fields, int32_t M, int32_t F, int32_t nb, const int32_t* starts,
                               const int32_t* places, const int64_t* field_ptr, int64_t N, uint64_t seed, uint64_t mc_seed,
                               int32_t nsamples, const dv_measure_params* params, double* mean_fields, double* stddev_fields,
                               double* residual_fields, double* mse_center, double* flux, double* flux_err, double* shape,
                               int32_t* iters, int32_t* status, double* flux_mean, double* flux_std, double* shape_mean,
                               double* shape_std, int32_t* n_ok, double* sample_flux, double* sample_shape,
                               int32_t* sample_status);

/* ---- blendedness: the share of its neighbours in the light under a galaxy's weight ----
 * Float64 throughout.  For galaxy i of field m: P its mean stamp [cs][cs][nb] (float32 widened), {r0, c0, Mrr, Mrc, Mcc} and
 * status its row of the measurement above, (pr, pc) = places[i], T the composited mean field of m ([F][F][nb]: the sum of all
 * mean stamps of m in object order, the bits of dv_infer_fields_composite), D the observed field of m.  The row is eligible
 * iff status is 0 or 2, the five shape values are finite and det = Mrr Mcc - Mrc^2 is finite and above 1e-6; an ineligible
 * row gets blend = 4 NaN and npix = -1.  Otherwise, over the stamp pixels (r, c) with 0 <= pr + r < F and 0 <= pc + c < F
 * (the pixels the composite keeps), with dr = r - r0, dc = c - c0 and
 *   g = exp(qa dr^2 + qb dr dc + qc dc^2), qa = -Mcc / (2 det), qb = Mrc / det, qc = -Mrr / (2 det):
 *   blend[i] = {W, A, Bm, Bd} = {sum g, sum g P[r,c,band], sum g T[pr+r,pc+c,band], sum g D[pr+r,pc+c,band]},
 *   npix[i] = the number of pixels summed (0, with four zero sums, for a stamp wholly outside its field).
 * The four sums visit the pixels with the same assignment to threads, round every product and sum on its own and reduce
 * in one fixed order: a galaxy's row has the same bits wherever it sits in a batch, and for a galaxy alone in its field A
 * and Bm have the same bits.  blendedness = 1 - A / Bm and blendedness_data = 1 - A / Bd are left to the caller.
 * dv_scene_blend: host arrays; stamps [N][cs][cs][nb] float32, shape [N][5], status [N], places [N][2], field_ptr [M + 1]
 * (stamps field_ptr[m] .. field_ptr[m + 1] lie in field m), model_fields and data_fields [M][F][F][nb]; data_fields may be
 * null (Bd is NaN on every row); blend [N][4], npix [N].  Chunked against free device memory.
 * dv_infer_fields_measure_blend: dv_infer_fields_measure (same arguments, same bits in every output it shares with it) with
 * blend / npix as one more stage: A and W behind the measurement of every chunk, Bm and Bd once a field's composite is
 * complete; T is the call's mean field, D the source field.  places is always needed.  In the catalogue-only form (the
 * three field outputs null) the mean field is still composited in device memory (one more resident field per field); it is
 * never downloaded.  The rows have the bits of dv_scene_blend on dv_infer_fields' stamps, dv_infer_fields_measure's rows
 * and dv_infer_fields_composite's mean fields.  Refused before any GPU work (DV_E_INVALID): by
 * dv_infer_fields_measure_blend what dv_infer_fields_measure refuses and a null places, blend or npix; by dv_scene_blend cs
 * or nb outside 1 .. 4096 (the kernels keep nothing per pixel: no LDS bound), band outside 0 .. nb - 1, a missing array, a
 * field_ptr that does not run from 0 to N without decreasing (checked whole before anything is indexed by it), a placement
 * beyond +-2^28. */
int dv_scene_blend(dv_ctx* ctx, const float* stamps, const double* shape, const int32_t* status, const int32_t* places,
                   const int64_t* field_ptr, int64_t N, int32_t cs, int32_t nb, int32_t band, const double* model_fields,
                   const double* data_fields, int32_t M, int32_t F, double* blend, int32_t* npix);
int dv_infer_fields_measure_blend(dv_model* m, const double* fields, int32_t M, int32_t F, int32_t nb, const int32_t* starts,
                                  const int32_t* places, const int64_t* field_ptr, int64_t N, uint64_t seed,
                                  const dv_measure_params* params, double* mean_fields, double* stddev_fields,
                                  double* residual_fields, double* mse_center, double* flux, double* flux_err, double* shape,
                                  int32_t* iters, int32_t* status, double* blend, int32_t* npix);

/* ---- PSF-corrected shapes: re-Gaussianization (Hirata & Seljak 2003) ----
 * Float64 throughout.  Per PSF image Q [ps][ps] (not necessarily normalised), once per call: the adaptive-moments iteration
 * of the measurement above on Q, from the centre and the width psf_sigma0, with the call's tol and max_iter, gives
 * psf_shape[k] = {q0r, q0c, Mrr, Mrc, Mcc}, psf_iters[k], psf_status[k]; psf_aux[k] = {A_P, FQ, psf_rho4} with FQ = sum Q,
 * A_P = sum g_P Q / sum g_P^2 (g_X the Gaussian weight of X's moments, as in the measurement) and rho4 as below (A_P and
 * psf_rho4 are NaN where psf_status is 3 or det M_P is not above 1e-6); eps[j] = (Q[j] - A_P g_P(j)) / FQ.  A PSF is usable
 * iff psf_status is 0, FQ is finite and positive and det M_P > 1e-6.
 * Per galaxy i: I = band `band` of its mean stamp, {r0, c0, M_I} = shape[i] and status[i] its row of the measurement,
 * psf_index[i] its PSF.  regauss_status[i] is 4 when the row is ineligible (status neither 0 nor 2, a value that is not
 * finite, det M_I not above 1e-6), 5 when psf_index[i] is outside 0 .. K - 1 or the PSF is not usable, 6 when
 * M_0 = M_I - M_P has Mrr <= 0 or det <= 1e-6 (the galaxy is not resolved); such a row gets six NaN and 0 iterations.
 * Otherwise A_I = sum g_I I / sum g_I^2, F0 = 2 pi sqrt(det M_I) A_I, f0(d) = F0 / (2 pi sqrt(det M_0)) exp(-d^T M_0^-1 d / 2),
 *   I'(x) = I(x) - sum_j eps[j] f0(x - (r0, c0) - (j - q0)), j over the ps^2 PSF pixels in row-major order,
 * and the iteration of the measurement on I', started from (r0, c0, M_I), gives regauss[i] = {r', c', Mrr', Mrc', Mcc',
 * rho4}, regauss_iters[i] and regauss_status[i] (0 / 2 / 3 as there), with, at the final state,
 *   rho4 = sum e^(-rho^2 / 2) I' rho^4 / sum e^(-rho^2 / 2) I', rho^2 = (Mcc dr^2 - 2 Mrc dr dc + Mrr dc^2) / det
 * (2 for a Gaussian; NaN on status 3 or a denominator that is not positive).  The corrected moments M' - M_P, and sigma, e1,
 * e2 and the resolution 1 - tr M_P / tr M' from them, are left to the caller.  A row has the same bits wherever it sits in
 * a batch.
 * dv_scene_regauss: host arrays; stamps [N][cs][cs][nb] float32, shape [N][5], status [N], psf_index [N], psf [K][ps][ps];
 * regauss [N][6], regauss_iters [N], regauss_status [N], psf_shape [K][5], psf_aux [K][3], psf_iters [K], psf_status [K].
 * Chunked against free device memory; the PSFs are uploaded and measured once.
 * dv_infer_fields_measure_psf: dv_infer_fields_measure (same arguments, same bits in every output it shares with it) with the
 * correction as one more stage behind every chunk's measurement; the new outputs have the bits of dv_scene_regauss on
 * dv_infer_fields' stamps and dv_infer_fields_measure's rows.  The catalogue-only form (three null field outputs) works as
 * there.  Refused before any GPU work (DV_E_INVALID): what dv_infer_fields_measure refuses; a null psf or a null output;
 * K < 1; ps outside 5 .. 33; cs above 64 (a thread keeps at most 16 pixels of I' in registers; every (cs, ps) within these
 * bounds fits a workgroup's LDS); psf_sigma0 not finite and positive.  A psf_index out of range is the row's status 5, not
 * a refusal. */
int dv_scene_regauss(dv_ctx* ctx, const float* stamps, const double* shape, const int32_t* status, const int32_t* psf_index,
                     int64_t N, int32_t cs, int32_t nb, int32_t band, const double* psf, int32_t K, int32_t ps,
                     double psf_sigma0, double tol, int32_t max_iter, double* regauss, int32_t* regauss_iters,
                     int32_t* regauss_status, double* psf_shape, double* psf_aux, int32_t* psf_iters, int32_t* psf_status);
int dv_infer_fields_measure_psf(dv_model* m, const double* fields, int32_t M, int32_t F, int32_t nb, const int32_t* starts,
                                const int32_t* places, const int64_t* field_ptr, int64_t N, uint64_t seed,
                                const dv_measure_params* params, double* mean_fields, double* stddev_fields,
                                double* residual_fields, double* mse_center, double* flux, double* flux_err, double* shape,
                                int32_t* iters, int32_t* status, const double* psf, int32_t K, int32_t ps,
                                const int32_t* psf_index, double psf_sigma0, double* regauss, int32_t* regauss_iters,
                                int32_t* regauss_status, double* psf_shape, double* psf_aux, int32_t* psf_iters,
                                int32_t* psf_status);

/* ---- aperture photometry: circular apertures, Kron flux and radius, flux radii ----
 * Float64 throughout; every expression is evaluated in the order written, each operation rounded on its own (no fused
 * multiply-add), with + - * /, comparisons and the correctly rounded square root only.  Per galaxy i: P its mean stamp
 * [cs][cs][nb] and S its stddev stamp (float32 widened), {r0, c0, Mrr, Mrc, Mcc} = shape[i] and status[i] its row of the
 * measurement in band `band`, I = P[:,:,band].  aper_status[i] is 4 when the row is ineligible (status neither 0 nor 2, a
 * value that is not finite, det = Mrr Mcc - Mrc Mrc not finite or not above 1e-6): every float output of the row is NaN and
 * aper_flags[i] is 0.  Otherwise, with dr = r - r0, dc = c - c0, o_i = (i + 0.5) / s - 0.5 for i = 0 .. s - 1 (s = subsample),
 * the weight of pixel (r, c) in a region inside(x, y) is w = #{(i, j): inside(dr + o_i, dc + o_j)} / (s s); circle k is
 * x x + y y <= R_k R_k, the ellipse of radius rho is q(x, y) = (a x) x + (b x) y + (c y) y <= rho rho with a = Mcc / det,
 * b = (-2 Mrc) / det, c = Mrr / det.  Every sum below runs over the pixels of the stamp whose weight is positive, and the
 * weight is carried as its count n: sum w x is (sum n x) / (s s), one division per sum, and sum w adds whole numbers, so an
 * area has the same bits in any order of summation.
 *   1. ap_flux[i][k][b] = sum w_k P[r,c,b], ap_flux_err[i][k][b] = sqrt(sum w_k (S[r,c,b] S[r,c,b])), ap_area[i][k] = sum w_k.
 *   2. Over the pixel centres with q(dr, dc) <= kron_limit kron_limit: r1 = sum sqrt(q) I / sum I.  If sum I is not finite or
 *      not positive, or r1 is not finite, aper_status[i] is 7 and everything under 2 - 4 is NaN (the circles are still given).
 *      rho_auto = kron_factor r1, or kron_min where that is smaller.
 *   3. The ellipse of radius rho_auto gives flux_auto[i][b], flux_auto_err[i][b] and auto_area; kron[i] = {r1, rho_auto,
 *      auto_area}.
 *   4. F(rho) = sum w_rho I, t_j = f_j flux_auto[i][band]; from lo = 0, hi = rho_auto, bisect_iters times: mid = 0.5 (lo + hi),
 *      F(mid) >= t_j ? hi = mid : lo = mid; flux_rho[i][j] = hi, in units of the moment ellipse (times det^(1/4): circularised
 *      pixels).
 * aper_flags[i]: bit k < 8 circle k leaves the stamp (r0 - R_k < -0.5, r0 + R_k > cs - 0.5, or the same for c0); bit 8 the
 * automatic ellipse does (half-extents rho_auto sqrt(Mrr), rho_auto sqrt(Mcc)); bit 9 the kron_limit ellipse does; bit 10
 * kron_min decided rho_auto.  Pixels outside the stamp do not exist: a flagged aperture is truncated.  A row has the same bits
 * wherever it sits in a batch.
 * dv_scene_aperture: host arrays; mean and stddev [N][cs][cs][nb] float32, shape [N][5], status [N]; ap_flux / ap_flux_err
 * [N][K][nb], ap_area [N][K], flux_auto / flux_auto_err [N][nb], kron [N][3], flux_rho [N][J], aper_flags / aper_status [N].
 * stddev, ap_flux_err and flux_auto_err are null together; with n_radii = 0 the three ap_ outputs may be null, with
 * n_fractions = 0 flux_rho.  Chunked against half of free device memory.
 * dv_infer_fields_measure_aper: dv_infer_fields_measure (same arguments, same bits in every output it shares with it) with the
 * photometry as one more stage behind every chunk's measurement, on the chunk's mean and stddev stamps in device memory; the
 * new outputs have the bits of dv_scene_aperture on dv_infer_fields' stamps and dv_infer_fields_measure's rows.  The
 * catalogue-only form (three null field outputs) works as there.
 * Refused before any GPU work (DV_E_INVALID): what dv_infer_fields_measure refuses (dv_scene_aperture: the same limits on
 * cs, nb and band); null params; a missing output; n_radii outside 0 .. 8 or n_fractions outside 0 .. 4; a radius that is not
 * finite and positive; a fraction not strictly between 0 and 1; subsample outside 1 .. 9; bisect_iters outside 1 .. 60;
 * kron_factor, kron_min or kron_limit not finite and positive. */
typedef struct dv_aperture_params {
  int32_t n_radii;         /* K, 0 .. 8 (3) */
  int32_t n_fractions;     /* J, 0 .. 4 (3) */
  int32_t subsample;       /* sub-pixels per pixel side, 1 .. 9 (5) */
  int32_t bisect_iters;    /* halvings per flux radius, 1 .. 60 (32) */
  double radii[8];         /* aperture radii in pixels (3, 5, 8) */
  double fractions[4];     /* flux fractions (0.2, 0.5, 0.8) */
  double kron_factor;      /* rho_auto = kron_factor r1 (2.5) */
  double kron_min;         /* the smallest rho_auto (3.5) */
  double kron_limit;       /* r1 is taken inside this ellipse (6.0) */
} dv_aperture_params;
int dv_aperture_params_default(dv_aperture_params* params);
int dv_scene_aperture(dv_ctx* ctx, const float* mean, const float* stddev, const double* shape, const int32_t* status,
                      int64_t N, int32_t cs, int32_t nb, int32_t band, const dv_aperture_params* params, double* ap_flux,
                      double* ap_flux_err, double* ap_area, double* flux_auto, double* flux_auto_err, double* kron,
                      double* flux_rho, int32_t* aper_flags, int32_t* aper_status);
int dv_infer_fields_measure_aper(dv_model* m, const double* fields, int32_t M, int32_t F, int32_t nb, const int32_t* starts,
                                 const int32_t* places, const int64_t* field_ptr, int64_t N, uint64_t seed,
                                 const dv_measure_params* params, double* mean_fields, double* stddev_fields,
                                 double* residual_fields, double* mse_center, double* flux, double* flux_err, double* shape,
                                 int32_t* iters, int32_t* status, const dv_aperture_params* aper, double* ap_flux,
                                 double* ap_flux_err, double* ap_area, double* flux_auto, double* flux_auto_err, double* kron,
                                 double* flux_rho, int32_t* aper_flags, int32_t* aper_status);

/* ---- aperture photometry on the observed field with the neighbours subtracted ----
 * The apertures above are sums over the network's own stamp P.  The same apertures on the observed field less the neighbours'
 * models, sum w (D - T + P), split as the blendedness sums do: sum w P is ap_flux, the rest needs the completed composite T
 * and the observed field D.  Float64 throughout, evaluated as above.  Per galaxy i of field m: shape[i], status[i] its row of
 * the measurement, kron[i] and aper_status[i] its row of the aperture photometry (rho_auto = kron[i][1]), (pr, pc) =
 * places[i], T = model_fields[m] and D = data_fields[m], both [F][F][nb].  The regions, the sub-pixel weights and their counts
 * n are those of section 7o about (r0, c0) in stamp coordinates; the sums run over the stamp pixels (r, c), 0 <= r, c < cs, of
 * positive count whose field pixel (pr + r, pc + c) lies inside the field - the pixels the composite keeps:
 *   ap_model_sum[i][k][b] = (sum n T[pr+r,pc+c,b]) / (s s), ap_data_sum[i][k][b] the same of D, ap_field_area[i][k] = (sum n) / (s s)
 *   auto_model_sum[i][b], auto_data_sum[i][b], auto_field_area[i]: the same three in the ellipse of radius rho_auto.
 * A row with aper_status 4, or that the eligibility test of section 7o refuses, is NaN in all six; a row whose aper_status is
 * not 0 is NaN in the three auto_ outputs (7: the circles are given).  A stamp wholly outside its field gives zero sums and
 * zero areas.  Without data_fields the two _data_sum outputs are NaN.  A row has the same bits wherever it sits in a batch;
 * for a galaxy alone in its field whose stamp does not leave it, ap_model_sum has the bits of ap_flux and auto_model_sum those
 * of flux_auto; where D and T hold the same bits, so do the data and model sums.
 * dv_scene_aperture_fields: host arrays; shape [N][5], status [N], places [N][2], field_ptr [M + 1] (stamps field_ptr[m] ..
 * field_ptr[m + 1] lie in field m), kron [N][3], aper_status [N], model_fields [M][F][F][nb], data_fields the same or null;
 * ap_model_sum / ap_data_sum [N][K][nb], ap_field_area [N][K], auto_model_sum / auto_data_sum [N][nb], auto_field_area [N];
 * with n_radii = 0 the three ap_ outputs may be null.  No stamp is an input.  Chunked against free device memory.
 * dv_infer_fields_measure_aper_data: dv_infer_fields_measure_aper (same arguments, same bits in every output it shares with
 * it) plus the six outputs, taken once a field's composite is complete from the catalogue rows, the aperture rows, the
 * placements, the mean field and the source field where they lie in device memory; they have the bits of
 * dv_scene_aperture_fields on those rows, dv_infer_fields_composite's mean fields and the source fields as data.  places is
 * always needed: in the catalogue-only form the mean field is composited on the device and never downloaded.
 * Refused before any GPU work (DV_E_INVALID): what dv_scene_aperture / dv_infer_fields_measure_aper refuse; a missing input or
 * output; a null places; F outside 1 .. 32768; a field_ptr that does not run from 0 to N or that decreases (the whole table is
 * checked before anything is indexed by it); a placement beyond +-2^28. */
int dv_scene_aperture_fields(dv_ctx* ctx, const double* shape, const int32_t* status, const int32_t* places,
                             const int64_t* field_ptr, const double* kron, const int32_t* aper_status, int64_t N, int32_t cs,
                             int32_t nb, const double* model_fields, const double* data_fields, int32_t M, int32_t F,
                             const dv_aperture_params* params, double* ap_model_sum, double* ap_data_sum,
                             double* ap_field_area, double* auto_model_sum, double* auto_data_sum, double* auto_field_area);
int dv_infer_fields_measure_aper_data(dv_model* m, const double* fields, int32_t M, int32_t F, int32_t nb,
                                      const int32_t* starts, const int32_t* places, const int64_t* field_ptr, int64_t N,
                                      uint64_t seed, const dv_measure_params* params, double* mean_fields,
                                      double* stddev_fields, double* residual_fields, double* mse_center, double* flux,
                                      double* flux_err, double* shape, int32_t* iters, int32_t* status,
                                      const dv_aperture_params* aper, double* ap_flux, double* ap_flux_err, double* ap_area,
                                      double* flux_auto, double* flux_auto_err, double* kron, double* flux_rho,
                                      int32_t* aper_flags, int32_t* aper_status, double* ap_model_sum, double* ap_data_sum,
                                      double* ap_field_area, double* auto_model_sum, double* auto_data_sum,
                                      double* auto_field_area);

/* ---- simultaneous flux fit of the deblended models to the observed field ----
 * Every flux above takes the network's amplitudes on trust, or corrects one galaxy while its neighbours stay at theirs.  Here
 * the shapes are held fixed and all the amplitudes of a field are fitted to the observed pixels at once, per band: linear
 * least squares, float64 throughout, every product and every sum rounded on its own.  Per field m with galaxies i = 0 .. n - 1
 * in object order: P_i the mean stamp [cs][cs][nb] (float32, widened), (pr_i, pc_i) = places[i], D = data_fields[m]
 * [F][F][nb].  The pixels of i are the stamp pixels whose field pixel lies inside the field - the pixels the composite keeps.
 * Per band b, independently:
 *   1. G_ij = sum P_i P_j over the field pixels both stamps cover, exactly 0.0 where the two clipped rectangles do not
 *      intersect; h_i = sum P_i D over the pixels of i.  Each sum is one fixed-order workgroup reduction.
 *   2. A galaxy whose G_ii is not finite or not positive gets fit_status 4 (DV_FIT_INELIGIBLE) in this band: fit_scale and
 *      fit_var NaN, not part of the system.
 *   3. Cholesky factorisation of G over the eligible galaxies in object order.  At column k the pivot is d_k = G_kk -
 *      sum_{j < k, kept} L_kj^2; d_k <= min_pivot G_kk drops galaxy k, fit_status 5 (DV_FIT_DROPPED).  A dropped column is
 *      never applied to the others: the variable leaves the system.  Of two models that cannot be told apart the one dropped
 *      is always the later one in object order.
 *   4. A dropped galaxy keeps the network's amplitude: h'_i = h_i - sum_{k dropped} G_ik; it reports fit_scale 1, fit_var NaN.
 *   5. G_kept a = h' by the two triangular solves.  fit_scale = a; fit_var_i = (G_kept^-1)_ii, the sum of squares of column i
 *      of L^-1 (times the sky variance per pixel it is the variance of fit_scale); fit_gram = G_ii and fit_proj = h_i are
 *      given for every galaxy.  Amplitudes are not clipped: a linear fit may return a negative one.  fit_status 0: fitted.
 * All five outputs are [N][nb].  A field's rows have the same bits wherever the field sits in a batch and when it is alone.
 * The Gram matrices of a field are dense, nb n n doubles in a scratch of at most params->scratch_bytes that the fields go
 * through in sub-ranges (no bit depends on the split); a field of more than DV_FIT_MAX_N galaxies is refused.
 * dv_scene_fit_flux: host arrays; stamps [N][cs][cs][nb] float32, places [N][2], field_ptr [M + 1] (stamps field_ptr[m] ..
 * field_ptr[m + 1] lie in field m), data_fields [M][F][F][nb].  Whole fields at a time, chunked against free device memory.
 * dv_infer_fields_measure_fit: dv_infer_fields_measure (same arguments, same bits in every output it shares with it) plus
 * the params and the five outputs: the mean stamps of every chunk are kept in device memory, and once a field's composite is
 * complete the fit runs on them, the placements and the source field where they lie.  The outputs have the bits of
 * dv_scene_fit_flux on dv_infer_fields_keep's mean stamps and the source fields.  places is always needed, with and without
 * the three result fields.
 * Refused before any GPU work (DV_E_INVALID, the engine stays usable): what dv_scene_blend refuses about field_ptr and the
 * placements; nb above 16; a missing array; min_pivot outside (0, 1); scratch_bytes < 1; a field of more than DV_FIT_MAX_N
 * galaxies and a field whose nb n n doubles exceed scratch_bytes - both messages name the field and its count. */
#define DV_FIT_MAX_N 1024
#define DV_FIT_INELIGIBLE 4
#define DV_FIT_DROPPED 5
typedef struct dv_fit_flux_params {
  double min_pivot;        /* relative pivot under which a galaxy is dropped; default 1e-8 */
  int64_t scratch_bytes;   /* device memory for the dense Gram matrices; default 256 MiB */
} dv_fit_flux_params;
int dv_fit_flux_params_default(dv_fit_flux_params* p);
int dv_scene_fit_flux(dv_ctx* ctx, const float* stamps, const int32_t* places, const int64_t* field_ptr, int64_t N, int32_t cs,
                      int32_t nb, const double* data_fields, int32_t M, int32_t F, const dv_fit_flux_params* params,
                      double* fit_scale, double* fit_var, double* fit_gram, double* fit_proj, int32_t* fit_status);
/* dv_scene_fit_flux_gram: step 1 alone for the n galaxies of ONE field, for a caller that wants the whole normal matrix (the
 * covariance between neighbours is sky_sigma^2 times the inverse of its kept part) - gram [nb][n][n], G_ij at [b][i][j] for
 * j <= i and 0.0 above the diagonal, proj [n][nb] = h.  Same sums, same bits as inside dv_scene_fit_flux.  Refuses what it
 * refuses, n above DV_FIT_MAX_N included. */
int dv_scene_fit_flux_gram(dv_ctx* ctx, const float* stamps, const int32_t* places, int64_t n, int32_t cs, int32_t nb,
                           const double* data_field, int32_t F, double* gram, double* proj);
int dv_infer_fields_measure_fit(dv_model* m, const double* fields, int32_t M, int32_t F, int32_t nb, const int32_t* starts,
                                const int32_t* places, const int64_t* field_ptr, int64_t N, uint64_t seed,
                                const dv_measure_params* params, double* mean_fields, double* stddev_fields,
                                double* residual_fields, double* mse_center, double* flux, double* flux_err, double* shape,
                                int32_t* iters, int32_t* status, const dv_fit_flux_params* fit, double* fit_scale,
                                double* fit_var, double* fit_gram, double* fit_proj, int32_t* fit_status);
/* The same fit under per-pixel weights.  weight_fields [M][F][F][nb] float64, laid out like the data
 * fields, is meant as the inverse variance of every pixel.  A pixel of band b COUNTS iff 0 < W < inf: zero, negative, infinite
 * and NaN weights all mask it, its terms are exactly +0.0 by selection, and nothing under it - a NaN in the data included -
 * reaches a sum.  No host pass validates W.  Step 1 becomes G_ij = sum (W P_i) P_j and h_i = sum (W P_i) D over the counting
 * pixels (the product with W first; with W = 1.0 everywhere every term has the bits of the unweighted one); steps 2 - 5 are
 * unchanged, so a galaxy without a counting pixel has fit_status 4, and fit_var IS the variance of fit_scale.  Two more
 * outputs [N][nb]: fit_npix, the number of counting pixels of the galaxy in the band (0 for a stamp wholly outside or wholly
 * masked), and fit_chi2 = sum over them of (W r) r with r = D - sum_j a_j P_j, j in ascending row order over the galaxies of
 * the field that cover the pixel and do not have fit_status 4, a_j = fit_scale (1 for a dropped galaxy); NaN where the galaxy
 * itself has fit_status 4.  dv_infer_fields_measure_fit_weighted keeps the weight fields resident beside the source fields (one
 * more field-sized buffer per resident field); its outputs have the bits of dv_scene_fit_flux_weighted on
 * dv_infer_fields_keep's mean stamps.  Both refuse what the unweighted calls refuse, and a null weight_fields, fit_chi2 or
 * fit_npix, before any GPU work (DV_E_INVALID, the engine stays usable). */
int dv_scene_fit_flux_weighted(dv_ctx* ctx, const float* stamps, const int32_t* places, const int64_t* field_ptr, int64_t N,
                               int32_t cs, int32_t nb, const double* data_fields, const double* weight_fields, int32_t M,
                               int32_t F, const dv_fit_flux_params* params, double* fit_scale, double* fit_var, double* fit_gram,
                               double* fit_proj, int32_t* fit_status, double* fit_chi2, int32_t* fit_npix);
int dv_infer_fields_measure_fit_weighted(dv_model* m, const double* fields, int32_t M, int32_t F, int32_t nb,
                                         const int32_t* starts, const int32_t* places, const int64_t* field_ptr, int64_t N,
                                         uint64_t seed, const dv_measure_params* params, double* mean_fields,
                                         double* stddev_fields, double* residual_fields, double* mse_center, double* flux,
                                         double* flux_err, double* shape, int32_t* iters, int32_t* status,
                                         const dv_fit_flux_params* fit, const double* weight_fields, double* fit_scale,
                                         double* fit_var, double* fit_gram, double* fit_proj, int32_t* fit_status,
                                         double* fit_chi2, int32_t* fit_npix);
/* The same fit by blend groups: no limit on the galaxies of a field.  Two galaxies of a field are
 * ADJACENT iff their stamp rectangles, clipped to the field, intersect (a stamp wholly outside its field is adjacent to
 * nothing, itself included); a BLEND GROUP is a connected component of that graph.  The groups depend on the placements alone,
 * not on the band, the weights or eligibility.  Two more outputs [N] int32: fit_group, the smallest row of the galaxy's group
 * counted from the first row of its field, and fit_group_size, the members of that group.  The neighbours are listed and the
 * components labelled on the GPU (an ordered compaction and min-label propagation with pointer jumping: no result depends on
 * the order of the threads); the host takes the labels, 4 bytes per galaxy, and orders the groups of a field by fit_group, the
 * members of a group staying in ascending row order.  Steps 1 - 5 (and the chi-square of the weighted fit) then run per group
 * as they run per field above: a group is the unit of scratch, nb n_g n_g doubles, and of solve workgroup; the field stays
 * the unit of data_fields and weight_fields.  Galaxies of different groups share no term, so on a field the dense calls take,
 * every output has the bits of dv_scene_fit_flux (weight_fields NULL; fit_chi2 and fit_npix NULL with it) or
 * dv_scene_fit_flux_weighted, as long as the factors are finite.  Refused before any GPU work (DV_E_INVALID, the engine stays
 * usable): what those two calls refuse except the count per field, a missing fit_group or fit_group_size, chi-square outputs
 * that do not match the weights.  Refused behind the labelling and before any solve (DV_E_INVALID, the stream idle, the engine
 * usable): a group of more than DV_FIT_MAX_N galaxies - "field f: the blend group of row r has n galaxies, the grouped fit
 * takes at most 1024 per group" - and a group whose nb n_g n_g doubles exceed scratch_bytes; both name the field, the group's
 * first row (counted from the field's first row) and its size.
 * dv_infer_fields_measure_fit_groups: dv_infer_fields_measure_fit_weighted with weight_fields nullable (fit_chi2 and fit_npix
 * NULL exactly then) plus the two outputs, at the completed-field seam on the same stamp store, with and without the result
 * fields: the bits of dv_scene_fit_flux_groups on dv_infer_fields_keep's mean stamps.  The group refusals come from the seam:
 * the catalogue rows of the call are then not delivered.
 * dv_scene_fit_groups: the groups alone from the placements - no stamps, no fit, no limit on a group - and, where pairs, adj_ptr
 * and adj are all given, the lists the fit works from, in rows of the call: pairs [n_pairs][2], the adjacent (i, j <= i) sorted
 * by i and then j, and the CSR adjacency adj_ptr [N + 1] / adj [n_adj] with ascending lists.  n_pairs and n_adj are always
 * written; lists shorter than them (pair_cap, adj_cap entries) are refused, so a caller asks twice. */
int dv_scene_fit_flux_groups(dv_ctx* ctx, const float* stamps, const int32_t* places, const int64_t* field_ptr, int64_t N,
                             int32_t cs, int32_t nb, const double* data_fields, int32_t M, int32_t F,
                             const dv_fit_flux_params* params, const double* weight_fields, double* fit_scale, double* fit_var,
                             double* fit_gram, double* fit_proj, int32_t* fit_status, double* fit_chi2, int32_t* fit_npix,
                             int32_t* fit_group, int32_t* fit_group_size);
int dv_infer_fields_measure_fit_groups(dv_model* m, const double* fields, int32_t M, int32_t F, int32_t nb, const int32_t* starts,
                                       const int32_t* places, const int64_t* field_ptr, int64_t N, uint64_t seed,
                                       const dv_measure_params* params, double* mean_fields, double* stddev_fields,
                                       double* residual_fields, double* mse_center, double* flux, double* flux_err, double* shape,
                                       int32_t* iters, int32_t* status, const dv_fit_flux_params* fit, const double* weight_fields,
                                       double* fit_scale, double* fit_var, double* fit_gram, double* fit_proj, int32_t* fit_status,
                                       double* fit_chi2, int32_t* fit_npix, int32_t* fit_group, int32_t* fit_group_size);
int dv_scene_fit_groups(dv_ctx* ctx, const int32_t* places, const int64_t* field_ptr, int64_t N, int32_t cs, int32_t M, int32_t F,
                        int32_t* fit_group, int32_t* fit_group_size, int64_t pair_cap, int64_t* n_pairs, int32_t* pairs,
                        int64_t adj_cap, int64_t* n_adj, int32_t* adj_ptr, int32_t* adj);
/* The same fit with a sky background fitted jointly: q terms per field and band beside the amplitudes,
 * sky_order 0: q = 1, a constant; sky_order 1: q = 3, a plane.  Per field of side F and pixel (r, c): B_0 = 1, B_1 = (double)
 * (2 r - F + 1) / (double)F, B_2 = (double)(2 c - F + 1) / (double)F; the model is D(p) = sum_i a_i P_i(p) + sum_t s_t B_t(p)
 * over ALL pixels of the field - with weight_fields the counting ones, masked terms selected to +0.0 as above; weight_fields
 * may be NULL, the unweighted fit.  Beside G and h of step 1: E_it = sum over the pixels of i of (W P_i) B_t, and per field
 * K_tu = sum (W B_t) B_u (u <= t), c_t = sum (W B_t) D and sky_npix, the counting pixels of the field (F F unweighted), summed
 * in a fixed tiling that depends on F alone.  The unknowns are the eligible galaxies in object order, then the sky terms: [[G,
 * E], [E^T, K]] [a; s] = [h; c], steps 2 - 5 as above.  The sky is eliminated last: fit_status, fit_gram and fit_proj of the
 * galaxies have the bits of the fit without sky.  A sky term whose K_tt is not finite or not positive has sky_status 4 (a
 * wholly masked field), coefficient and covariance NaN; one whose pivot d <= min_pivot K_tt has sky_status 5: its coefficient
 * is exactly 0.0, it is never applied to the others and nothing is subtracted from the right-hand side for it.  Dropped
 * galaxies keep amplitude 1 in the sky rows too: c'_t = c_t - sum_{k dropped} E_kt.  fit_var now carries the covariance with
 * the sky.  A field without galaxies is still solved: its sky is the (weighted) mean or plane of D.  fit_chi2 (weighted calls
 * only): M(p) gains sum_t s_t B_t(p) after the neighbours, t ascending, over the terms with sky_status 0.  Unweighted, a
 * non-finite pixel of D anywhere in the field now reaches every galaxy of the field through the sky; weight_fields mask it.
 * Outputs: the seven galaxy outputs of the weighted calls - fit_chi2 and fit_npix are NULL exactly when weight_fields is -,
 * then per field sky_coef [M][nb][q], sky_cov [M][nb][q][q] (the lower-right block of the inverse; NaN in the rows and columns
 * of terms that are not kept), sky_status [M][nb][q] and sky_npix [M][nb] int64.  A field's outputs have the same bits
 * wherever it sits in a batch.  The scratch of a field is nb (n + q) (n + q) doubles.  Both calls refuse, before any GPU work
 * (DV_E_INVALID, the engine stays usable), what the weighted calls refuse, a sky_order outside {0, 1}, a missing sky output
 * and chi-square outputs that do not match the weights.
 * dv_scene_fit_flux_sky_gram: step 1 of the bordered system of ONE field - gram [nb][n + q][n + q], the lower triangle of
 * [[G, E], [E^T, K]] and 0.0 above the diagonal, rhs [n + q][nb] = h, c: the bits the solve starts from. */
int dv_scene_fit_flux_sky(dv_ctx* ctx, const float* stamps, const int32_t* places, const int64_t* field_ptr, int64_t N, int32_t cs,
                          int32_t nb, const double* data_fields, const double* weight_fields, int32_t M, int32_t F,
                          const dv_fit_flux_params* params, int32_t sky_order, double* fit_scale, double* fit_var, double* fit_gram,
                          double* fit_proj, int32_t* fit_status, double* fit_chi2, int32_t* fit_npix, double* sky_coef,
                          double* sky_cov, int32_t* sky_status, int64_t* sky_npix);
int dv_scene_fit_flux_sky_gram(dv_ctx* ctx, const float* stamps, const int32_t* places, int64_t n, int32_t cs, int32_t nb,
                               const double* data_field, const double* weight_field, int32_t F, int32_t sky_order, double* gram,
                               double* rhs);
int dv_infer_fields_measure_fit_sky(dv_model* m, const double* fields, int32_t M, int32_t F, int32_t nb, const int32_t* starts,
                                    const int32_t* places, const int64_t* field_ptr, int64_t N, uint64_t seed,
                                    const dv_measure_params* params, double* mean_fields, double* stddev_fields,
                                    double* residual_fields, double* mse_center, double* flux, double* flux_err, double* shape,
                                    int32_t* iters, int32_t* status, const dv_fit_flux_params* fit, const double* weight_fields,
                                    int32_t sky_order, double* fit_scale, double* fit_var, double* fit_gram, double* fit_proj,
                                    int32_t* fit_status, double* fit_chi2, int32_t* fit_npix, double* sky_coef, double* sky_cov,
                                    int32_t* sky_status, int64_t* sky_npix);
/* The non-negative fit: the same quadratic minimised subject to a_i >= 0 for every galaxy, the sky terms
 * left free - what scarlet and the Tractor solve; clipping the negative amplitudes of the linear fit afterwards leaves the
 * neighbours biased.  sky_order -1: no sky, and sky_coef, sky_cov, sky_status and sky_npix must all be NULL; 0 / 1 as above.
 * weight_fields may be NULL, and fit_chi2 and fit_npix are NULL exactly then.  Iteration 1 is the fit above: it fixes
 * fit_status, the dropped set (amplitude 1), h' and the unconstrained amplitudes.  With Z the clamped galaxies (empty at
 * first), p = 3 and best = n + 1, iteration t = 1, 2, ...: factorise G over the kept unknowns not in Z (no pivot test after
 * iteration 1) and solve for a, a_i = +0.0 in Z; y_i = (sum_j G_ij a_j) - h'_i for i in Z, j ascending over the kept unknowns
 * not in Z, sky terms included; V = {kept galaxies not in Z with a_i < 0} + {i in Z with y_i < 0}, strict; V empty: converged.
 * Otherwise, |V| < best: best = |V|, p = 3, every member of V changes sides; else p > 0: p -= 1, every member changes sides;
 * else the largest index of V alone does.  After max_iter (>= 1) iterations with V not empty the rows hold the last solved
 * iterate - negative amplitudes may remain - and nonneg_status is 1.  fit_var, sky_cov and fit_chi2 come from the last
 * iteration; fit_var is NaN for a clamped galaxy.  Outputs: those of the sky calls - fit_scale exactly +0.0 where clamped;
 * fit_gram, fit_proj and fit_status with the bits of the unconstrained fit - then fit_scale_free [N][nb], the fit_scale of the
 * unconstrained call, bit for bit; fit_clamped [N][nb] int32, 0 or 1; fit_dual [N][nb], y_i where clamped, +0.0 where
 * passive, NaN for status 4 or 5; and per field nonneg_iters [M][nb] int32, the factorisations (1: the unconstrained fit was
 * feasible, and every output shared with the calls above has their bits; 0: no unknowns), and nonneg_status [M][nb] int32, 0
 * converged, 1 max_iter reached.  Both calls refuse, before any GPU work (DV_E_INVALID, the engine stays usable), what the sky
 * and weighted calls refuse, max_iter < 1, a missing new output and sky outputs given with sky_order -1. */
int dv_scene_fit_flux_nonneg(dv_ctx* ctx, const float* stamps, const int32_t* places, const int64_t* field_ptr, int64_t N,
                             int32_t cs, int32_t nb, const double* data_fields, const double* weight_fields, int32_t M, int32_t F,
                             const dv_fit_flux_params* params, int32_t sky_order, int32_t max_iter, double* fit_scale,
                             double* fit_var, double* fit_gram, double* fit_proj, int32_t* fit_status, double* fit_chi2,
                             int32_t* fit_npix, double* sky_coef, double* sky_cov, int32_t* sky_status, int64_t* sky_npix,
                             double* fit_scale_free, int32_t* fit_clamped, double* fit_dual, int32_t* nonneg_iters,
                             int32_t* nonneg_status);
int dv_infer_fields_measure_fit_nonneg(dv_model* m, const double* fields, int32_t M, int32_t F, int32_t nb, const int32_t* starts,
                                       const int32_t* places, const int64_t* field_ptr, int64_t N, uint64_t seed,
                                       const dv_measure_params* params, double* mean_fields, double* stddev_fields,
                                       double* residual_fields, double* mse_center, double* flux, double* flux_err, double* shape,
                                       int32_t* iters, int32_t* status, const dv_fit_flux_params* fit, const double* weight_fields,
                                       int32_t sky_order, int32_t max_iter, double* fit_scale, double* fit_var, double* fit_gram,
                                       double* fit_proj, int32_t* fit_status, double* fit_chi2, int32_t* fit_npix, double* sky_coef,
                                       double* sky_cov, int32_t* sky_status, int64_t* sky_npix, double* fit_scale_free,
                                       int32_t* fit_clamped, double* fit_dual, int32_t* nonneg_iters, int32_t* nonneg_status);

/* ---- adaptive moments on the observed field with the neighbours subtracted ----
 * The measurement of dv_scene_measure on the CHILD IMAGE of every galaxy instead of on the network's mean stamp.  Per galaxy i
 * of field m: P_i [cs][cs][nb] float32 its mean stamp, (pr, pc) = places[i] its place, T = model_fields[m] and D =
 * data_fields[m], both [F][F][nb] float64, and optionally W = weight_fields[m] of the same shape (NULL: none).  Stamp pixel
 * (r, c), band b lies on field pixel (R, Cc) = (pr + r, pc + c).  The pixel COUNTS iff it lies inside the field and, where W is
 * given, 0 < W[R, Cc, b] < inf (the rule of the weighted flux fit: a NaN or saturated value of D under a masked pixel reaches
 * nothing).  Child image: C_i[r, c, b] = (D[R, Cc, b] - T[R, Cc, b]) + (double)P_i[r, c, b] where the pixel counts - two
 * roundings in that order, no contraction - and (double)P_i[r, c, b] elsewhere: the model fills in what the field edge or the
 * mask hides.  Outputs: flux_data [N][nb] = the sum of C_i[., ., b] over the whole stamp, in the thread assignment and
 * reduction order of dv_scene_measure's flux; npix_data [N][nb] int32 = the counting pixels; shape_data [N][5], iters_data [N]
 * and status_data [N] = the adaptive-moments iteration of dv_scene_measure on the float64 plane C_i[:, :, band], from the stamp
 * centre and sigma0^2 I, with the same status codes.  A non-finite D at a counting pixel of `band` ends in status 3 and is not
 * hidden.  A stamp wholly outside its field has npix_data 0 and C = P: it gets the model's row.  Where D has the bits of T,
 * every output has the bits of dv_scene_measure on the same stamps.  The weights are a mask only: the moments are not
 * inverse-variance weighted.  A galaxy's outputs have the same bits wherever it sits in a batch.
 * dv_scene_moments_fields: host arrays in and out, whole fields at a time within free device memory; field_ptr [M + 1] as in
 * dv_scene_fit_flux.  Refused before any GPU work (DV_E_INVALID, the engine stays usable): what dv_scene_measure refuses (band,
 * sigma0, tol, max_iter, a stamp above 90 pixels), a missing input or output, a null places, a bad field_ptr (checked whole
 * before anything is indexed by it), F outside 1 .. 32768, a placement beyond +-2^28.
 * dv_infer_fields_measure_moments_data: dv_infer_fields_measure plus weight_fields [M][F][F][nb] (nullable) and the five
 * outputs, taken at the completed-field seam from the mean stamps the chunk loop has kept, with and without the result fields
 * (the catalogue-only form composites T on the device and needs places too): the bits of dv_scene_moments_fields on
 * dv_infer_fields_keep's mean stamps, dv_infer_fields_composite's mean fields and the source fields. */
int dv_scene_moments_fields(dv_ctx* ctx, const float* stamps, const int32_t* places, const int64_t* field_ptr, int64_t N,
                            int32_t cs, int32_t nb, const double* model_fields, const double* data_fields,
                            const double* weight_fields, int32_t M, int32_t F, const dv_measure_params* params,
                            double* flux_data, int32_t* npix_data, double* shape_data, int32_t* iters_data, int32_t* status_data);
int dv_infer_fields_measure_moments_data(dv_model* m, const double* fields, int32_t M, int32_t F, int32_t nb,
                                         const int32_t* starts, const int32_t* places, const int64_t* field_ptr, int64_t N,
                                         uint64_t seed, const dv_measure_params* params, double* mean_fields,
                                         double* stddev_fields, double* residual_fields, double* mse_center, double* flux,
                                         double* flux_err, double* shape, int32_t* iters, int32_t* status,
                                         const double* weight_fields, double* flux_data, int32_t* npix_data, double* shape_data,
                                         int32_t* iters_data, int32_t* status_data);

/* ---- resident field sets: iterative deblending with the fields on the GPU ----
 * dv_field_set_open uploads M float64 fields [M][F][F][nb] once; the set (owned by the model: dv_model_destroy frees it)
 * keeps per field, in device memory, `work` (what the next pass detects on and cuts from, at first the field), `final`
 * (the field minus every stamp of every pass so far), `mean` and `stddev` (sums over all passes), and in reference mode
 * (cumulative = 0) `base`, the field as uploaded.  The whole set is resident: M fields times 6 buffers (4 in cumulative
 * mode, where `final` is `work`) must fit 80 % of free device memory less a reserve for what the passes allocate (the
 * inference pipeline, the detector's workspace, the per-stamp tables), or DV_FIELDS_GROUP_MB if that is lower, else
 * DV_E_NOMEM before any GPU work (a set never splits itself: the noise rows would change).  nb must be the network's.
 * dv_field_set_detect: dv_scene_detect on band 2 of `work` (nb >= 3) for the fields with active[m] != 0 (NULL: all), gathered
 * on the GPU; the catalogue of dv_scene_detect without maps, `field` and offsets [M + 1] in the set's numbering, an
 * inactive field has an empty range and globalrms 0.  Same bits as dv_scene_detect on the fields read back.
 * dv_field_set_pass: one deblending pass.  starts, places [N][2], field_ptr [M + 1] and seed as in
 * dv_infer_fields_composite; the stamps are cut from `work` as it is before the pass.  For every field m that has stamps,
 * in object order and in float64: work_new = (cumulative ? work : base) - mean stamps, final -= mean stamps, mean += mean
 * stamps, stddev += stddev stamps, field_mse[m] = mean((work - work_new)^2) over the F * F * nb elements, then work =
 * work_new.  Fields without stamps are untouched and their field_mse entry is not written.  mse_center [N] is
 * dv_infer_fields_composite's.  The sums have the bits of dv_scene_composite on dv_infer_fields' stamps; field_mse is
 * summed in a fixed order of its own (blocks of 2048 elements, a fixed tree): the same bits on every run, for any M and
 * whatever the other fields hold, but not numpy's.  The refusals of dv_infer_fields_composite apply, before any GPU work,
 * and leave the set as it was.
 * dv_field_set_read copies one of the stacks to out [M][F][F][nb].  dv_field_set_close frees the device memory; every
 * call on a closed set returns DV_E_STATE (the handle stays valid until its model is destroyed: a closed set keeps ~150
 * bytes of host memory with its model, so a model that opens many sets in its life grows by that much per set). */
#define DV_FIELD_SET_WORK 0
#define DV_FIELD_SET_FINAL 1
#define DV_FIELD_SET_MEAN 2
#define DV_FIELD_SET_STDDEV 3
int dv_field_set_open(dv_model* m, const double* fields, int32_t M, int32_t F, int32_t nb, int32_t cumulative,
                      dv_field_set** out);
int dv_field_set_detect(dv_field_set* set, const uint8_t* active, const dv_detect_params* params, int64_t cap,
                        int64_t* n_out, int64_t* offsets, double* globalrms, int32_t* field, int32_t* parent,
                        int32_t* npix, double* peak, double* flux, double* x, double* y);
/* dv_field_set_detect_weights: weights [M][F][F] float64 (one plane per field, for band 2), noise and
 * filter as in dv_scene_detect_weighted.  The planes are uploaded once and stay with the set until dv_field_set_close or a
 * call with weights = NULL, which drops them; their M * F * F * 8 bytes are counted against free device memory
 * (DV_E_NOMEM, the set left as it was).  While planes are held dv_field_set_detect takes the weighted path: the bits of
 * dv_scene_detect_weighted on band 2 of `work` read back and the planes of the active fields; a field without a good mesh
 * has an empty range and globalrms NaN.  With no planes held it is as above.  With absolute noise dv_field_set_detect
 * refuses thresh <= 0.  Refused (DV_E_INVALID): an unknown noise or filter; a closed set: DV_E_STATE. */
int dv_field_set_detect_weights(dv_field_set* set, const double* weights, int32_t noise, int32_t filter);
/* dv_field_set_detect_bands: the band selection of dv_scene_detect_multiband for every later
 * dv_field_set_detect, which then takes the multi-band path on `work` (the bits of dv_scene_detect_multiband on `work` read
 * back).  bands [k], band_weights [k] or NULL, planes [M][F][F][k] or NULL with noise, filter as there; the planes are uploaded
 * once, counted against free device memory like those of dv_field_set_detect_weights (DV_E_NOMEM, the set left as it was).
 * k = 0 drops the selection and its planes.  Refused (DV_E_INVALID): what dv_scene_detect_multiband refuses of these
 * arguments, and a selection while single-band planes of dv_field_set_detect_weights are held (which in turn is refused
 * while a selection is held); a closed set: DV_E_STATE. */
int dv_field_set_detect_bands(dv_field_set* set, const int32_t* bands, int32_t k, const double* band_weights,
                              const double* planes, int32_t noise, int32_t filter);
/* dv_field_set_detect_objects: on != 0: every later dv_field_set_detect also computes the columns of
 * dv_scene_detect_objects (segmap_on != 0: and the segmap) and the set keeps those of its last detection on the host;
 * dv_field_set_detect itself keeps its signature and its outputs.  on = 0 drops them.
 * dv_field_set_detect_objects_read copies them out: the non-null columns of `out` [n_expected], rows as in the catalogue of
 * that detection, and segmap [M][F][F] in the set's numbering, 0 in fields that were not active.  Refused (DV_E_INVALID):
 * the switch off, no detection kept (none since the switch went on, or its catalogue did not fit its cap), n_expected
 * other than that detection's *n_out, a segmap asked for with segmap_on = 0, a null `out`; a closed set: DV_E_STATE.  While
 * the switch is on dv_field_set_detect refuses thresh < 0. */
int dv_field_set_detect_objects(dv_field_set* set, int32_t on, int32_t segmap_on);
int dv_field_set_detect_objects_read(dv_field_set* set, int64_t n_expected, const dv_detect_objects* out);
/* dv_field_set_detect_clean: on != 0: every later dv_field_set_detect (same signature) runs the
 * cleaning pass of dv_scene_detect_clean with clean_param and returns the cleaned catalogue; the set keeps nmerged, mthresh
 * and n_raw of its last detection on the host, and the columns of dv_field_set_detect_objects, when that switch is on, are
 * the cleaned ones.  on = 0 drops them: the detection is the one it was.  dv_field_set_detect_clean_read copies out the
 * non-null nmerged, mthresh [n_expected] and n_raw [M] (0 for a field that was not active).  Refused (DV_E_INVALID): on != 0
 * with clean_param not finite or <= 0; reading with the switch off, with no detection kept or with n_expected other than
 * that detection's *n_out; a closed set: DV_E_STATE.  While the switch is on dv_field_set_detect refuses thresh <= 0 and
 * minarea > 64. */
int dv_field_set_detect_clean(dv_field_set* set, int32_t on, double clean_param);
int dv_field_set_detect_clean_read(dv_field_set* set, int64_t n_expected, int32_t* nmerged, double* mthresh, int64_t* n_raw);
int dv_field_set_pass(dv_field_set* set, const int32_t* starts, const int32_t* places, const int64_t* field_ptr, int64_t N,
                      uint64_t seed, double* mse_center, double* field_mse);
int dv_field_set_read(dv_field_set* set, int32_t which, double* out);
int dv_field_set_close(dv_field_set* set);

/* ---- the catalogue of the iterative loop, measured on the resident set ----
 * dv_field_set_pass_measure: dv_field_set_pass (same arguments, same bits in the stacks, mse_center and field_mse) with two
 * more stages behind every chunk's forward pass, on the chunk's mean and stddev stamps in device memory: the measurement
 * above (flux, flux_err [N][nb], shape [N][5], iters, status [N]: the bits of dv_scene_measure on the stamps dv_infer_fields
 * returns for the working residuals and the same seed) and the child sums of the blendedness (child [N][2] = {W, A}, npix
 * [N]: the bits of dv_scene_blend's W, A and npix for those stamps, rows and placements).  child and npix may be null
 * TOGETHER: no child sums are taken.  With them given the set appends {shape[5], status, place, field} of every stamp to
 * resident rows it owns in device memory, in call order (the first stamp of a pass follows the last stamp of the pass
 * before); they grow like the per-stamp tables, never cross the host link again and are freed by dv_field_set_close.
 * Refused before any GPU work (DV_E_INVALID), the set and its resident rows left as they were: what dv_field_set_pass and
 * dv_infer_fields_measure refuse (a stamp of more than 90 pixels among it), null params, child without npix or npix without
 * child.
 * dv_field_set_blend: for all Ntot resident rows, against the set's stacks as they are at the time of the call (usually:
 * after the last pass), with the pixels, the weight g and the eligibility rule of the blendedness above and pr, pc, field
 * the row's: sums [Ntot][4] = {Bm, Bd, R1, R2} = {sum g mean, sum g base, sum g final, sum g (final final)} at band `band`,
 * the square rounded on its own.  Bm and Bd have the bits of dv_scene_blend's on the stacks read back (base is the field as
 * uploaded).  A cumulative set keeps no `base`: Bd is NaN on every row.  An ineligible row gets four NaN.  In reference
 * mode a galaxy deblended again in a later pass is in `mean` once per pass: its Bm counts its earlier copies as neighbours.
 * n_expected must be Ntot, the number of stamps of all passes that took child sums (DV_E_INVALID otherwise, and for a band
 * outside 0 .. nb - 1), so that a caller whose rows and the set's have come apart learns it before it joins them. */
int dv_field_set_pass_measure(dv_field_set* set, const int32_t* starts, const int32_t* places, const int64_t* field_ptr,
                              int64_t N, uint64_t seed, const dv_measure_params* params, double* mse_center,
                              double* field_mse, double* flux, double* flux_err, double* shape, int32_t* iters,
                              int32_t* status, double* child, int32_t* npix);
int dv_field_set_blend(dv_field_set* set, int32_t band, int64_t n_expected, double* sums);

/* ---- the joint flux fit of all passes of the iterative loop ----
 * dv_field_set_keep_stamps(set, on): from now on a dv_field_set_pass_measure call that keeps resident rows (child and npix
 * given) also keeps the pass's float32 mean stamps in device memory, each at its resident row number; they grow with the
 * rows and are freed by dv_field_set_close.  Allowed only while the set holds no resident rows (DV_E_STATE otherwise, and on
 * a closed set).  With the switch off every other call queues what it queued before and returns the same bits.
 * dv_field_set_fit_flux: ONE linear system per field and band over the models of EVERY pass - the fit of dv_scene_fit_flux,
 * _weighted, _sky or _nonneg, chosen by weight (NULL: unweighted), sky_order (-1: none, 0, 1) and nonneg - against `data`
 * [M][F][F][nb] (host), or with data NULL against the fields as uploaded (reference mode only: a cumulative set keeps no
 * copy, DV_E_INVALID).  Inside a field the galaxies stand in resident-row order, pass ascending and then the in-pass order:
 * of two models that cannot be told apart the copy from the LATER pass is dropped (status 5, scale 1).  The set's rows are
 * regrouped field by field in device memory and run through the kernels of the stand-alone calls: every output has the bits
 * of the stand-alone call on the same stamps regrouped the same way.  Per-row outputs [Ntot][nb] are in resident-row (call)
 * order; the sky outputs and nonneg_iters / nonneg_status are per field as in the stand-alone calls.  An output the chosen
 * variant does not produce must be NULL, one it produces must not.  The call reads the set and never writes it: it may be
 * repeated.  Zero rows: returns at once.  Refused before any GPU work, the set left as it was: n_expected is not Ntot
 * (DV_E_INVALID); a closed set, or stamps never kept (DV_E_STATE); sky_order outside -1 .. 1; what the stand-alone calls
 * refuse of params, nb above 16 among it; nonneg_max_iter < 1 with nonneg; a field whose scratch exceeds scratch_bytes; a
 * field of more than DV_FIT_MAX_N galaxies summed over its passes (the message names the field and the count). */
int dv_field_set_keep_stamps(dv_field_set* set, int32_t on);
int dv_field_set_fit_flux(dv_field_set* set, int64_t n_expected, const double* data, const double* weight, int32_t sky_order,
                          int32_t nonneg, const dv_fit_flux_params* params, int32_t nonneg_max_iter, double* fit_scale,
                          double* fit_var, double* fit_gram, double* fit_proj, int32_t* fit_status, double* fit_chi2,
                          int32_t* fit_npix, double* sky_coef, double* sky_cov, int32_t* sky_status, int64_t* sky_npix,
                          double* fit_scale_free, int32_t* fit_clamped, double* fit_dual, int32_t* nonneg_iters,
                          int32_t* nonneg_status);

/* ---- the joint flux fit of all passes by blend groups ----
 * dv_field_set_fit_flux_groups: the fit of dv_scene_fit_flux_groups on the rows of EVERY pass - the rows of the set in the joint
 * order of dv_field_set_fit_flux (field by field, inside a field pass ascending and then the in-pass order), the blend groups
 * the connected components of the overlap graph of that order, every group solved on its own.  fit_group [Ntot] is the
 * smallest row of the galaxy's group counted from the field's first row IN THE JOINT ORDER - an index into the field's rows
 * concatenated pass after pass -, fit_group_size [Ntot] the members of that group; inside a group the copy from the LATER pass
 * is the one dropped (status 5, scale 1).  The fit works in place on the stamp store: only the placements and fields of the
 * rows are regrouped, there is no second copy of the stamps.  `data` and `weight` [M][F][F][nb] (host) as in
 * dv_field_set_fit_flux: weight NULL is the unweighted fit, data NULL the fields as uploaded (reference mode only); fit_chi2
 * and fit_npix are NULL iff weight is.  Every output is in resident-row (call) order and has the bits of
 * dv_scene_fit_flux_groups on the same stamps regrouped field by field, and - where that call takes the field - of
 * dv_field_set_fit_flux.  No sky, no constraint.  A field may hold any number of rows.  The call reads the set and never writes
 * it: it may be repeated.  Zero rows: returns at once.  Refused before any solve, the set left as it was and usable: n_expected
 * is not Ntot (DV_E_INVALID); a closed set, or stamps never kept (DV_E_STATE); what dv_scene_fit_flux_groups refuses of params
 * and nb; a blend group of more than DV_FIT_MAX_N galaxies or whose nb x n_g x n_g doubles exceed scratch_bytes (the message
 * names the field, the group's first row and the count); DV_E_NOMEM where the tables, the scratch, the rows and the uploaded
 * fields exceed free device memory. */
int dv_field_set_fit_flux_groups(dv_field_set* set, int64_t n_expected, const double* data, const double* weight,
                                 const dv_fit_flux_params* params, double* fit_scale, double* fit_var, double* fit_gram,
                                 double* fit_proj, int32_t* fit_status, double* fit_chi2, int32_t* fit_npix, int32_t* fit_group,
                                 int32_t* fit_group_size);

/* ---- introspection for tests and bench ----------------------------------------------------- */
/* copy a named activation of the last step to host: "t","z","kl","eps","loc","scale","head_pre" */
int dv_model_get_activation(dv_model* m, const char* name, float* host, size_t nbytes);
/* HIP-event timing of kernel classes on the engine stream: class 0 gconv, 1 wgrad, 2 everything else */
int dv_prof_enable(dv_model* m, int32_t on);
int dv_prof_read(dv_model* m, int32_t klass, int64_t* launches, double* total_ms);
int dv_prof_reset(dv_model* m);
/* the same timing per MFMA kernel family (fam = 0 .. until DV_E_INVALID): `name` is the kernel name rocprofv3 prints
 * (without template arguments), flops the algorithmic FLOPs of the timed launches (padding taps counted),
 * executed_flops what the matrix pipe executes for them (a Winograd kernel: 16 multiplies per 2 x 2 tile and channel pair
 * instead of 36, over blocks / column tiles padded to its geometry; direct kernels: the algorithmic count),
 * algorithmic_bytes the HBM bytes of the launches with every operand read once and every result written once (0 for
 * families that do not report them).  Any out pointer may be NULL. */
int dv_prof_read_family(dv_model* m, int32_t fam, char* name, size_t name_len, int64_t* launches, double* total_ms,
                        double* flops, double* executed_flops, double* algorithmic_bytes);

#if defined(__GNUC__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif /* DEBVADER_HIP_H */
