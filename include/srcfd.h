/* srcfd.h -- C ABI of libsrcfd.so, the MI355X-native super-resolution engine.
 *
 * Drop-in boundary for ONE hot path of bitseal02/SR-for-CFD: the 10x10 ->
 * 400x400 convolutional-autoencoder SR call.  The reference has no FFI layer;
 * its boundary is the Python surface the solver scripts call, so every entry
 * point below cites the reference call it replaces (paths relative to the
 * reference checkout).  INTEGRATION.md shows the ctypes binding.
 *
 * Conventions: plain C, no torch / STL types.  Every function returns an int
 * status (0 = SRCFD_OK, negative = error) unless noted, never throws, and
 * leaves a thread-local message readable through srcfd_last_error().
 * A handle is not thread-safe; distinct handles may be used from distinct
 * threads.  Compute entry points fail with SRCFD_ENODEV when no HIP device is
 * present -- there is no CPU fallback.
 * No entry point reads or writes caller memory outside the extents its comment
 * states, and every element of an output extent is written unless the comment
 * says otherwise (the stitch's "left as it was" for an index outside `y` is
 * such an exception).
 *
 * Device pointers (every argument named *_dev).  Each is a DENSE, C-ordered array of the stated element type and
 * shape on the handle's device.  No strides cross this ABI: a strided view (one channel of an interleaved tensor, a
 * transposed view, every other row) is read or written as if it were dense, so a caller makes it contiguous first.
 * Required alignment: that of the ELEMENT and nothing wider -- 4 bytes for float32 and int32, 2 bytes for a 16-bit
 * y_dev, 8 bytes for float64 and int64.  That is what a contiguous view into a larger allocation has (a row slice, an
 * offset into a flat buffer).  The kernels make 8- and 16-byte accesses at addresses derived from these pointers; all
 * of them are plain global loads, stores or atomics, which the device takes at any element alignment, and no caller
 * pointer goes into a buffer descriptor or an LDS-direct load.  No entry point returns SRCFD_EINVAL for an
 * element-aligned pointer.  Two launchers take a narrower path, with the same bits, when the pointers they are handed
 * share less than 16 bytes of alignment: srcfd_trainer_forward_backward[_ex] (two device-to-device copies instead of
 * the 16-byte staging kernel) and the stitch of srcfd_tiles_stitch_device / srcfd_tiler_run (vector width V, the
 * align_bytes of srcfd_tiled_plan).  Each entry point below repeats its own line.  The C side checks these pointers for
 * NULL only: it cannot see dtype, shape, strides or device.  The Python binding checks all four on every tensor before
 * it takes its address (_lib.device_ptr; ValueError, nothing enqueued).  Audit: DESIGN.md section 7; every entry point
 * at 1, 2 and 3 elements behind a 256-byte boundary: tests/test_gpu_device_args.py.
 */
#ifndef SRCFD_H
#define SRCFD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SRCFD_OK 0
#define SRCFD_ENOENT (-2)   /* file missing            -> Python FileNotFoundError (PyCFD_ML_accelerated.py:1080-1087) */
#define SRCFD_EIO (-5)      /* unreadable / malformed  -> Python OSError           (PyCFD_ML_accelerated.py:835-837)   */
#define SRCFD_ENOMEM (-12)
#define SRCFD_ENODEV (-19)  /* no HIP device / extension cannot run */
#define SRCFD_EINVAL (-22)
#define SRCFD_EKEY (-126)   /* missing key             -> Python KeyError          (PyCFD_ML_accelerated.py:822-825)   */
#define SRCFD_EHIP (-1000)  /* HIP runtime error, text in srcfd_last_error() */

typedef enum {
  SRCFD_F32 = 0, SRCFD_F64 = 1, SRCFD_I32 = 2, SRCFD_I64 = 3, SRCFD_U8 = 4, SRCFD_STR = 5,
  SRCFD_BF16 = 16, SRCFD_F16 = 17
} srcfd_dtype;

/* Arithmetic the network is evaluated in. */
typedef enum {
  SRCFD_PREC_FP32 = 0,       /* f32 MFMA (v_mfma_f32_32x32x2_f32), exact f32 products: parity path     */
  SRCFD_PREC_BF16 = 1,       /* bf16 operands, f32 accumulate, fused tail: throughput path             */
  SRCFD_PREC_FP32_NAIVE = 2, /* one thread per output, f32 FMA chain: bring-up / cross-check           */
  SRCFD_PREC_F16 = 3,        /* f16 operands, f32 accumulate (BASELINE config 5)                        */
  SRCFD_PREC_FP32X3 = 4      /* f32 storage and vector math; the wide decoder GEMMs (ConvT#0, ConvT#1) and the
                                streaming tail's first layer as six bf16 MFMAs on operands split exactly into
                                three bf16 terms (kernels_x3.hip, tail32<X3>): f32-grade results (<= 1e-5 vs the
                                float64 oracle, measured 5e-7) at 6/16 of the f32 matrix time, from 64 samples per
                                call on; smaller calls and everything else run the SRCFD_PREC_FP32 kernels.   */
} srcfd_precision;

typedef enum {
  SRCFD_LAYER_CONV2D = 1, SRCFD_LAYER_CONV2D_TRANSPOSE = 2, SRCFD_LAYER_DENSE = 3,
  SRCFD_LAYER_FLATTEN = 4, SRCFD_LAYER_RESHAPE = 5
} srcfd_layer_kind;

typedef enum { SRCFD_ACT_LINEAR = 0, SRCFD_ACT_SWISH = 1, SRCFD_ACT_RELU = 2, SRCFD_ACT_SIGMOID = 3, SRCFD_ACT_TANH = 4 } srcfd_activation;

/* One Keras layer (sr-ae-conv.ipynb:c162-169, c277-287).  Kernel layouts are
 * Keras': Conv2D (kh,kw,Cin,Cout); Conv2DTranspose (kh,kw,Cout,Cin); Dense
 * (in,out).  Pointers are host memory, copied at create.
 * same_padding, per axis with kernel k and stride s:
 *   Conv2D:           0 'valid': out = (in - k) / s + 1;  1 'same': out = ceil(in / s), TensorFlow's padding (the odd pixel goes after).
 *   Conv2DTranspose:  0 'valid': out = (in - 1) s + k, full[s i + a] += x[i] W[a] (no kernel flip);
 *                     1 'same':  out = in s, rows [pb, pb + in s) of that 'valid' result, pb = (k - s) / 2 (integer division);
 *                                bias and activation come after the crop.  k = 3, s = 2: pb = 0, the LAST row and column go.
 *                                k == s: the same layer as 'valid'.  k < s is refused at create / load. */
typedef struct {
  int kind;        /* srcfd_layer_kind */
  int activation;  /* srcfd_activation */
  int kh, kw, stride, same_padding; /* conv / conv-transpose */
  int cin, cout;   /* channels (Dense: in/out features) */
  int reshape[3];  /* RESHAPE target (h,w,c) */
  const float* kernel;
  const float* bias;
  const char* name; /* optional Keras layer name (used by srcfd_model_save_h5); NULL -> layer_<i> */
} srcfd_layer;

typedef struct srcfd_model srcfd_model;
typedef struct srcfd_h5 srcfd_h5;
typedef struct srcfd_h5w srcfd_h5w;
typedef struct srcfd_trainer srcfd_trainer;
typedef struct srcfd_resampler srcfd_resampler;

const char* srcfd_last_error(void);
const char* srcfd_version(void);
/* Number of HIP devices (0 on a CPU-only box; never an error). */
int srcfd_device_count(void);

/* ---- model lifetime ------------------------------------------------------
 * srcfd_model_load_h5 replaces the pair of
 *   tf.keras.models.load_model(encoder_file, compile=False)
 *   tf.keras.models.load_model(decoder_file, compile=False)
 * + SuperResolutionAE(encoder_lr, decoder_hr)   (PyCFD_ML_accelerated.py:831-833,
 * bfs_ml_accelerated.py:1069-1071): parses `model_config` and
 * `model_weights/<layer>/<layer>/{kernel,bias}` from legacy Keras-H5 files and
 * chains the sub-models.  Either path may be NULL to load one half.
 * device < 0 builds a host-only handle (shape queries / weight access only). */
int srcfd_model_load_h5(const char* encoder_h5, const char* decoder_h5, int device, srcfd_model** out);
/* Same from in-memory layers (tests, training hand-off). in_shape = (h,w,c). */
int srcfd_model_create(const srcfd_layer* layers, int n_layers, const int in_shape[3], int device, srcfd_model** out);
void srcfd_model_destroy(srcfd_model* m);

int srcfd_model_input_shape(const srcfd_model* m, int shape[3]);
int srcfd_model_output_shape(const srcfd_model* m, int shape[3]);
int srcfd_model_num_layers(const srcfd_model* m);
/* Layer i: fills *layer with pointers into the handle's host copy of the weights. */
int srcfd_model_get_layer(const srcfd_model* m, int i, srcfd_layer* layer, char* name, size_t name_len);
/* Multiply-accumulates per sample (140 024 128 for encoder_10+decoder_400). */
int64_t srcfd_model_macs_per_sample(const srcfd_model* m);
int srcfd_model_set_precision(srcfd_model* m, int precision);
int srcfd_model_get_precision(const srcfd_model* m);
/* Allocates now what the first n-sample forward at the CURRENT precision would allocate or pack lazily (activation
 * workspaces, 16-bit operand packs), so that a latency- or throughput-critical first call does no set-up work.  Optional:
 * every forward reserves what it needs itself.  The reference pays the equivalent cost inside its first
 * `predict` (graph tracing, PyCFD_ML_accelerated.py:858). */
int srcfd_model_reserve(srcfd_model* m, int n);
/* What an n-sample forward at `precision` keeps allocated, WITHOUT allocating anything (works on a host-only handle): bytes[0] device
 * activation workspace (what srcfd_model_reserve reserves), bytes[1] device weights and operand packs (upper bound), bytes[2] device
 * staging of the host-buffer entry (srcfd_predict), bytes[3] host bytes of one result of the call (page-locked when it comes from
 * srcfd_host_alloc).  For capacity planning of several ranks on one host (bench.py's dry run); the reference has no counterpart
 * (TensorFlow grows its arena on demand, PyCFD_ML_accelerated.py:858). */
int srcfd_model_footprint(const srcfd_model* m, int n, int precision, size_t bytes[4]);
/* 1 when the bf16/f16 fused decoder_400 kernels apply to this layer graph. */
int srcfd_model_has_fused_path(const srcfd_model* m);
/* 1 when srcfd_model_set_precision(m, precision) would be accepted (works on a host-only handle).  The f32 precisions: every graph.
 * SRCFD_PREC_BF16 / SRCFD_PREC_F16: the fused graph above, or a graph whose first four compute layers are encoder_10's, that ends
 * in a 3x3 stride-1 'same' Conv2D to ONE channel (linear, 16 .. 64 input channels, a multiple of 16) and whose layers in between are
 * Dense or 2x2 / 3x3 stride-2 Conv2DTranspose ('valid' or 'same'), swish or linear, input channels a multiple of 16: encoder_10 +
 * decoder_{10,20,50,80,100} of the notebook.  Those run layer by layer (srcfd_model_last_plan: decoder=any16). */
int srcfd_model_supports_precision(const srcfd_model* m, int precision);

/* ---- forward -------------------------------------------------------------
 * srcfd_predict replaces `inference_model.predict(x, verbose=0)`
 * (PyCFD_ML_accelerated.py:858, bfs_ml_accelerated.py:1109, sr-ae-conv.ipynb:c349):
 * x is float32 NHWC (n,h,w,c) C-contiguous host memory, y a caller-allocated
 * float32 (n,oh,ow,oc) host buffer.  Blocks until y is complete.
 *
 * Optional fused pre/post-processing, per sample i (both may be NULL):
 *   in_affine[2i..2i+1]  = (mean, std): x := (x - mean) / std in float32
 *       (standardize_with_stats, PyCFD_ML_accelerated.py:665-668; std==0 -> 1e-8)
 *   out_affine[2i..2i+1] = (mean, std): y := y * std + mean in float32
 *       (inverse_standardize, PyCFD_ML_accelerated.py:671-673).  SRCFD_PREC_FP32 (the parity path): two roundings,
 *       bit for bit numpy's float32 result; the 16-bit precisions fuse the two into ONE fma (<= 1 ulp from it)
 * flags: SRCFD_FLAG_NAN_GUARD zero-fills every element that is non-finite in y's own type and counts them in
 * *n_nonfinite (PyCFD_ML_accelerated.py:869-876): NaN, +-Inf, and with a 16-bit y (srcfd_predict_device) a float32
 * value that the round-to-nearest-even cast turns into +-Inf (|v| >= 65520 for float16).  A guarded call returns no
 * non-finite element (tests/test_gpu_nonfinite_guard.py). */
#define SRCFD_FLAG_NAN_GUARD 1
int srcfd_predict(srcfd_model* m, const float* x, int n, const float* in_affine, const float* out_affine,
                  float* y, int flags, int64_t* n_nonfinite);

/* Page-locked host memory for the arrays handed to srcfd_predict.  A result (y) that lives in such memory -- from here, or any
 * hipHostMalloc / hipHostRegister'ed range -- is filled at the PCIe rate with the copy of one chunk overlapping the kernels of the
 * next; a pageable result is staged by the runtime (about 45 GB/s, nothing overlaps) and, when freshly allocated, also pays its
 * first-touch page faults.  The Python surface keeps a recycling pool of these behind predict() (engine.py). */
int srcfd_host_alloc(size_t bytes, void** out);
void srcfd_host_free(void* p);

/* Device-resident variant for the batched path: x_dev float32 (n,h,w,c),
 * affines float32 device arrays or NULL, y_dev of dtype out_dtype (SRCFD_F32,
 * SRCFD_BF16 or SRCFD_F16), nonfinite_dev an optional device int64 counter
 * that is ADDED to.  Enqueues on hip_stream (a hipStream_t, NULL = default
 * stream) and returns without synchronising.
 * Pointers: x_dev dense (n,h,w,c), 4-byte aligned; the affines dense (n,2), 4-byte aligned; y_dev dense (n,oh,ow,oc),
 * aligned to its element (4 bytes, or 2 for the 16-bit types) although the last kernel stores 16 (f32) or 8 (16-bit) bytes
 * per lane; nonfinite_dev 8-byte aligned (a 64-bit atomic add).  y_dev must hold all n samples: the library cannot see its
 * size.  A call of more samples than srcfd_model_workspace reports runs in chunks at x_dev + i in_elems,
 * y_dev + i out_elems, affine row i, into the same counter.
 * One handle, one stream at a time: the activation workspace, the split-K slabs
 * and the captured hipGraph belong to the handle, so two calls on the SAME handle
 * are ordered only when they are enqueued on the same stream.  A caller that moves
 * a handle to another stream orders the two calls itself (an event, or a
 * synchronisation in between); nothing in the handle does.  Distinct handles may be
 * in flight on distinct streams at once (tests/test_gpu_stream_order.py). */
int srcfd_predict_device(srcfd_model* m, const void* x_dev, int n, const float* in_affine_dev,
                         const float* out_affine_dev, void* y_dev, int out_dtype, int flags,
                         int64_t* nonfinite_dev, void* hip_stream);
/* Largest n one srcfd_predict_device call processes without internal chunking
 * at the current precision, and the workspace bytes it holds for that. */
int srcfd_model_workspace(srcfd_model* m, int n, size_t* bytes);

/* Per-kernel timing of the last srcfd_predict_device call made with profiling
 * enabled: HIP events on the launch stream around every kernel.  names is a
 * '\n'-joined list; ms has one entry per name. */
int srcfd_model_set_profiling(srcfd_model* m, int enable);
int srcfd_model_get_profile(srcfd_model* m, char* names, size_t names_len, float* ms, int* count, int max_count);
/* Test hook: copies the first `bytes` of inter-kernel activation buffer `index`
 * (0 or 1) of the bf16/f16 pipeline to host memory after synchronising.  After a
 * forward, index 0 is ConvT#1's output (n,50,50,64), 16-bit, scaled by log2(e); index 1
 * is ConvT#0's (n,25,25,128) only when the generic GEMM path ran (env SRCFD_MID=0) --
 * the default fused ConvT#0->ConvT#1 kernel never materialises it. */
int srcfd_model_debug_activation(srcfd_model* m, int index, void* dst, size_t bytes);
/* Test hook: which implementation of each stage the handle's LAST forward ran, as "key=value" words separated by blanks, e.g.
 * "precision=bf16 encoder=enc16 dense_1=dense1_16 middle=mid16 tail=tail16 tail_seg=10 graph=replay".  The A/B switches SRCFD_ENC,
 * SRCFD_DENSE1, SRCFD_MID, SRCFD_TAIL (=s), SRCFD_NO_ENC32, SRCFD_NO_DENSE_SKINNY and SRCFD_TAIL_SEG are read from the environment on every
 * srcfd_predict* call; each selects a complete second implementation (the parity tests compare the two), none skips work, and a
 * captured hipGraph is replayed only under the switches it was captured with.  graph: eager | capture | replay. */
int srcfd_model_last_plan(const srcfd_model* m, char* buf, size_t buf_len);
/* Test hook: the steps an n-sample forward of the handle's f32-grade precision would take under the switches the environment holds
 * now, as "first-op-name=kernel:ops" words separated by blanks, e.g. "conv2d=enc32:4 dense_1=skinny:1 conv2d_transpose.ph00=big:4 ...".
 * kernel: enc32 | tail32 | triple | pair | x3 | big | group | skinny | finalize | mfma | naive (engine.h, F32Kernel).  Asks the same
 * function the launch loop asks; launches nothing and works on a host-only handle.  SRCFD_EINVAL under a 16-bit precision. */
int srcfd_model_f32_steps(const srcfd_model* m, int n, char* buf, size_t buf_len);

/* ---- stats file ----------------------------------------------------------
 * `key value` lines, '#' comments (PyCFD_ML_accelerated.py:787-797).  Looks up
 * mean{lr}_{c}, std{lr}_{c}, mean{hr}_{c}, std{hr}_{c} for c in u,v,p
 * (PyCFD_ML_accelerated.py:800-809) into out[12] = lr(u,v,p)x(mean,std) then
 * hr(u,v,p)x(mean,std).  SRCFD_ENOENT / SRCFD_EKEY as the reference raises. */
int srcfd_stats_load(const char* path, int lr_dim, int hr_dim, double out[12]);
/* Writer of the same format (sr-ae-conv.ipynb:c589-603). */
int srcfd_stats_save(const char* path, int lr_dim, int hr_dim, const double in[12]);

/* ---- HDF5 subset (legacy Keras-H5, solver field dumps) -------------------
 * Replaces h5py for this path: reads what `load_model` reads
 * (PyCFD_ML_accelerated.py:831-832) and the coarse-field files the solvers
 * write (PyCFD_ML_accelerated.py:517-544); writes the layout
 * `encoder.save(...h5)` produces (sr-ae-conv.ipynb:c584-586). */
int srcfd_h5_open(const char* path, srcfd_h5** out);
void srcfd_h5_close(srcfd_h5* f);
/* '\n'-joined child names of a group; *needed = bytes incl. terminator. */
int srcfd_h5_list(srcfd_h5* f, const char* group, char* buf, size_t buf_len, size_t* needed);
/* kind: 0 absent, 1 group, 2 dataset. */
int srcfd_h5_kind(srcfd_h5* f, const char* path);
int srcfd_h5_dataset_info(srcfd_h5* f, const char* path, int* dtype, int* rank, uint64_t dims[8]);
int srcfd_h5_read(srcfd_h5* f, const char* path, void* dst, size_t dst_bytes, int as_dtype);
/* String attribute ('\n'-joined when an array); numeric attribute as doubles. */
int srcfd_h5_attr_string(srcfd_h5* f, const char* obj, const char* name, char* buf, size_t buf_len, size_t* needed);
int srcfd_h5_attr_numeric(srcfd_h5* f, const char* obj, const char* name, double* out, int max_count, int* count);
int srcfd_h5_attr_names(srcfd_h5* f, const char* obj, char* buf, size_t buf_len, size_t* needed);

int srcfd_h5w_create(srcfd_h5w** out);
void srcfd_h5w_free(srcfd_h5w* w);
int srcfd_h5w_group(srcfd_h5w* w, const char* path);
int srcfd_h5w_dataset(srcfd_h5w* w, const char* path, int dtype, int rank, const uint64_t* dims, const void* data);
/* n_strings == 0 writes a scalar string attribute from strings[0]. */
int srcfd_h5w_attr_strings(srcfd_h5w* w, const char* obj, const char* name, const char* const* strings,
                           int n_strings, int is_scalar, int utf8);
int srcfd_h5w_attr_numeric(srcfd_h5w* w, const char* obj, const char* name, int dtype, const void* value, int count, int is_scalar);
int srcfd_h5w_save(srcfd_h5w* w, const char* path);
/* Saves the handle's weights as legacy Keras-H5 sub-model files
 * (sr-ae-conv.ipynb:c584-585); split_at = index of the first decoder layer. */
int srcfd_model_save_h5(const srcfd_model* m, const char* encoder_h5, const char* decoder_h5);
/* The whole-model file `superres_model.save("superres_{lr}to{hr}_vanilla_ae_{suffix}.h5")` (sr-ae-conv.ipynb:c586):
 * encoder and decoder in ONE legacy Keras-H5 file (groups model_weights/<sub-model>/<layer>/{kernel,bias}, the layout
 * Keras 3.8 writes for a subclassed Model; unpinned -- the reference's superres files are absent, .MISSING_LARGE_BLOBS:29-31).
 * Loading takes the architecture from the nested sub-model configs when the file carries them and otherwise assumes the
 * reference's encoder_10 / decoder_400 definition (sr-ae-conv.ipynb:c162-169, c277-287). */
int srcfd_model_save_superres_h5(const srcfd_model* m, const char* superres_h5);
int srcfd_model_load_superres_h5(const char* superres_h5, int device, srcfd_model** out);

/* ---- device-side resampling of the SR output (BFS aspect-ratio correction) -------------------
 * Replaces `reshape_square_to_rectangular` (bfs_ml_accelerated.py:104-145): per component
 * RectBivariateSpline(y_sq, x_sq, field, kx=3, ky=3)(y_rect, x_rect) is linear in `field` and
 * separable, i.e. out = Ry * field * Rx^T with the 1-D interpolating-spline matrices
 * Ry [out_h][in_h], Rx [out_w][in_w] (row-major float64, host; built once by the caller, see
 * sr-for-cfd_amd/resample.py).  The handle keeps them on `device`. */
int srcfd_resampler_create(int device, const double* Ry, const double* Rx, int in_h, int in_w, int out_h, int out_w,
                           srcfd_resampler** out);
void srcfd_resampler_destroy(srcfd_resampler* r);
/* in_dev float32 (n,in_h,in_w) -> out_dev float64 (n,out_h,out_w), enqueued on hip_stream.
 * Pointers: both dense; in_dev 4-byte, out_dev 8-byte aligned (element-wise loads and stores only). */
int srcfd_resample_device(srcfd_resampler* r, const float* in_dev, int n, double* out_dev, void* hip_stream);
/* The same for float64 input (a solver's fields, srcfd_fine_batch_get_fields_device): in_dev float64 (n,in_h,in_w), enqueued on
 * `stream` (a hipStream_t).  The same kernels instantiated for a float64 operand: the same two float64 products in the same
 * summation order, so for input values that are exactly floats the output equals srcfd_resample_device's bit for bit.
 * Pointers: both dense, 8-byte aligned. */
int srcfd_resample_device_f64(srcfd_resampler* r, const double* in_dev, int n, double* out_dev, void* stream);
/* srcfd_predict followed by the resampling, without the float32 result leaving the device:
 * `predict` + inverse standardise + NaN guard (bfs_ml_accelerated.py:1109-1127) + resample back
 * (:1130-1135).  y is float64 host (n,out_h,out_w), like scipy returns it. */
int srcfd_predict_resampled(srcfd_model* m, srcfd_resampler* r, const float* x, int n, const float* in_affine,
                            const float* out_affine, double* y, int flags, int64_t* n_nonfinite);

/* ---- input preparation on the device (batched BFS calls) ------------------------------------------
 * Replaces, per sample (one component of one coarse field), what `ml_super_resolution` does before `predict` in the BFS
 * solver: `reshape_rectangular_to_square` (bfs_ml_accelerated.py:59-101; X = Ry F Rx^T with the 1-D spline matrices
 * Ry [lr][h], Rx [lr][w], float64, DEVICE; both NULL = no resampling), `.astype(np.float32)` (:1086), and the adaptive
 * blend of the training statistics with np.mean / np.std of the float32 field (:1091-1097; adaptive = 0: the training
 * statistics as they are).  fields_dev float64 (n,h,w); train_stats_dev float64 (n,2) = (mean, std) of each sample's
 * component; writes x_dev float32 (n,lr,lr) [or (n,h,w)] and in_affine_dev float32 (n,2), the arguments
 * srcfd_predict_device takes.  Pointers: all dense; the float64 inputs (fields_dev, Ry_dev (lr,h), Rx_dev (lr,w), train_stats_dev)
 * 8-byte, x_dev and in_affine_dev 4-byte aligned (element-wise loads and stores only).  The statistics reproduce numpy's float32 arithmetic (pairwise sums, NumPy-2 scalar
 * promotion) bit for bit.  Sides up to 32. */
int srcfd_prepare_inputs_device(const double* fields_dev, int n, int h, int w, const double* Ry_dev, const double* Rx_dev, int lr,
                                const double* train_stats_dev, int adaptive, double blend, float* x_dev, float* in_affine_dev,
                                void* hip_stream);

/* ---- scoring: predictions against targets, on the device, with numpy's bits -------------------------
 * Replaces the reductions of `evaluate_for_re` (sr-ae-conv.ipynb:c323-369), the only accuracy numbers the reference publishes
 * (MAE and range-normalised MAE per component at the held-out Reynolds number).  Per sample, with float32 pred and truth of
 * `elems` elements and optional (mean, std) pairs:
 *   p = pred * std + mean, t = truth * std + mean   (inverse_standardize: two float32 roundings each, never an fma; no pair: the
 *                                                    value as it is);   d = t - p
 *   metrics[SRCFD_SCORE_MAE]       np.mean(np.abs(t - p))        metrics[SRCFD_SCORE_MSE]       np.mean((t - p)**2)
 *   metrics[SRCFD_SCORE_MAX_ABS]   np.max(np.abs(t - p))
 *   metrics[SRCFD_SCORE_TRUTH_MIN] np.min(t)                     metrics[SRCFD_SCORE_TRUTH_MAX] np.max(t)
 *   metrics[SRCFD_SCORE_PRED_MIN]  np.min(p)                     metrics[SRCFD_SCORE_PRED_MAX]  np.max(p)
 *   metrics[SRCFD_SCORE_NONFINITE] number of non-finite d, as a float (exact: elems <= 2^24)
 * Every value has the bit pattern numpy's float32 expression gives (tests/test_gpu_score.py), so a score does not depend on who
 * computed it.  Min and max are NaN when a NaN is present, as numpy's are; which of -0.0 and +0.0 an extreme is, where both
 * occur, is as little defined as it is in numpy.
 * The two means follow numpy's summation order, which is NOT one pairwise tree over the field:
 *   1. the flattened array is cut into consecutive chunks of 8192 elements (np.getbufsize()), the last one shorter;
 *   2. a chunk of n elements is summed by pairwise_sum: n < 8 serially from 0.f; 8 <= n <= 128 with eight accumulators
 *      r[j] = a[j], r[j] += a[i + j] for i = 8, 16, .. < n - n % 8, res = ((r0+r1)+(r2+r3)) + ((r4+r5)+(r6+r7)), then res += a[i]
 *      for the last n % 8 elements; n > 128: n2 = n / 2, n2 -= n2 % 8, pairwise(a, n2) + pairwise(a + n2, n - n2);
 *   3. res = 0.f; res += chunk sum, chunk by chunk;   4. mean = res / (float)elems.   Every operation float32, round to nearest.
 * elems: 1 .. 2 560 000 (1600 x 1600), else SRCFD_EINVAL.  One launch per call (one workgroup per sample), csrc/score.hip. */
#define SRCFD_SCORE_FIELDS 8
#define SRCFD_SCORE_MAE 0
#define SRCFD_SCORE_MSE 1
#define SRCFD_SCORE_MAX_ABS 2
#define SRCFD_SCORE_TRUTH_MIN 3
#define SRCFD_SCORE_TRUTH_MAX 4
#define SRCFD_SCORE_PRED_MIN 5
#define SRCFD_SCORE_PRED_MAX 6
#define SRCFD_SCORE_NONFINITE 7
/* Test hook: the summation order for a field of `elems` elements (csrc/score_plan.h), the tables the kernel reads, as JSON:
 * {"elems":E,"chunk":8192,"n_chunks":..,"full":{"leaves":[[off,len],..],"nodes":[[left,right,height],..]}|null,"last":{..}|null}
 * "full": a chunk of 8192, "last": the chunk of E % 8192.  "nodes" are the inner nodes, every one after its children; a child
 * index below len(leaves) names a leaf, any other nodes[index - len(leaves)].  Needs no device. */
int srcfd_score_plan(int64_t elems, char* buf, size_t len);
/* pred, truth: float32 (n, elems) host; affines float32 (n, 2) host or NULL; metrics float32 (n, SRCFD_SCORE_FIELDS) host.
 * Blocks until metrics is complete. */
int srcfd_score_fields(int device, const float* pred, const float* truth, int n, int64_t elems,
                       const float* pred_affine, const float* truth_affine, float* metrics);
/* A held-out set that stays on the device.  create uploads x (n, in_elems), truth (n, out_elems) and the affines ((n, 2) each, or
 * NULL) ONCE.  score predicts the set's x with m at m's current precision, in chunks of up to 256 samples (the chunks of
 * srcfd_predict into pageable memory, so every sample has the bits srcfd_predict of the whole set gives it), and scores every
 * chunk's device result against the resident truth; only the n x SRCFD_SCORE_FIELDS metrics cross to the host.  The forward
 * applies in_affine and nothing else (no out_affine, no NaN guard); the scorer applies pred_affine and truth_affine -- the
 * notebook's order, predict standardised, then inverse-standardise both -- so the metrics equal numpy's on
 * `model.predict(x)` in every precision (the 16-bit forwards fuse an out_affine into one fma and would not).
 * SRCFD_EINVAL when m's input or output element count is not the set's, or m is on another device.  m is left as it was
 * (weights, precision).  A set belongs to one device and score runs on m's workspace on the default stream: the rule "one
 * handle, one stream at a time" of srcfd_predict_device holds for m while score runs, and a set is not thread-safe. */
typedef struct srcfd_evalset srcfd_evalset;
int srcfd_evalset_create(int device, const float* x, int64_t in_elems, const float* truth, int64_t out_elems, int n,
                         const float* in_affine, const float* pred_affine, const float* truth_affine, srcfd_evalset** out);
int srcfd_evalset_score(srcfd_evalset* e, srcfd_model* m, float* metrics);
int srcfd_evalset_destroy(srcfd_evalset* e);

/* ---- tiled super-resolution on the device: cut, predict and stitch ---------------------------------
 * BASELINE config 5 without the host in between (the host form is pipeline.tiled_super_resolution; the reference defines no
 * tiling): a float32 coarse field (TY*lh, TX*lw, C), C-contiguous on the device, is cut into TY x TX tiles of the
 * model's input size; component c of tile (ty, tx) is sample s = (ty*TX + tx)*C + c of a ONE-channel model lh x lw -> hh x hw; the
 * samples' results are stitched into out (TY*hh, TX*hw, C), channel-interleaved, float32.  No overlap and no blending here (below: the overlapped form).  The two
 * kernels (csrc/tiles.hip) only move values: out has the bits of numpy's reshape / transpose of srcfd_predict's results.
 *
 * srcfd_tiled_plan (host only, needs no device): what a tiler of these sizes would do, as JSON --
 *   {"n":N,"chunk":K,"n_chunks":M,"chunks":[[first,count],..]|null,"v":V,"cut":{"grid":G,"block":256},
 *    "stitch":{"block":256,"items_per_tile":I,"blocks_per_tile":B,"grid":[one per chunk]|null},"intermediate_bytes":Y}
 * (lh, lw, in_channels) / (hh, hw, out_channels): the model's input / output shape.  K: the largest multiple of C not above
 * max_chunk when max_chunk > 0, else not above model_chunk (what srcfd_model_workspace returns for N samples), never below C: a
 * chunk never splits the C components of a tile.  V: floats per lane and source row of the stitch, the widest of 4, 2, 1 with
 * hw % V == 0 and align_bytes (the alignment of the stitch's two base pointers; 16 and more count as 16) a multiple of 4 V.
 * Y = K*hh*hw*4.  The two lists are null above 65536 chunks.  SRCFD_EINVAL with the reason: C outside 1 .. 8, TY or TX < 1, more
 * than INT_MAX samples, a model input or output of more than one channel.  The launch code executes exactly this plan.
 *
 * A srcfd_tiler belongs to one model handle (borrowed: once the model is destroyed, srcfd_tiler_destroy is the only call left)
 * and one (TY, TX, C, max_chunk); it owns the tile buffer, the per-sample affine arrays and the planar intermediate of one chunk.
 * create: SRCFD_ENODEV on a host-only model; the
 * chunk is sized from the model's precision at that moment (a later change of precision stays correct: srcfd_predict_device
 * chunks by itself).  max_chunk <= 0: none.
 * Streams: the stream is BOUND to the handle (set_stream; a hipStream_t, NULL = the default stream, which is also the initial
 * binding), not passed per call.  run, cut and stitch enqueue on it and return without synchronising.  "One handle, one stream at
 * a time" (srcfd_predict_device) holds for the tiler AND for the model it borrows: the tiler's buffers, the model's workspace
 * and its captured hipGraph are ordered only by that one stream; a caller that rebinds the stream, or uses the model elsewhere,
 * orders the two uses itself.  These entries take no per-call stream parameter, so the table of tests/test_gpu_stream_order.py
 * (built from the parameter name it looks for) does not list them; what the table stands for -- a side-stream test of every
 * stream-ordered entry point -- is met for srcfd_tiler_run, srcfd_tiles_cut_device and srcfd_tiles_stitch_device by
 * tests/test_gpu_tiled_device.py (test_side_stream_*).  A change of that table's rule should pick these three up.
 *
 * srcfd_tiler_run: cut, then per chunk srcfd_predict_device into the intermediate and a stitch of the chunk's tiles.
 * in_affine_dev / out_affine_dev: per-COMPONENT (C, 2) (mean, std) device arrays or NULL, applied as srcfd_predict applies row
 * s % C to sample s.  flags / nonfinite_dev: passed to every predict call (SRCFD_FLAG_NAN_GUARD; the counter is ADDED to).
 * srcfd_tiles_cut_device: the cut alone -- x_dev (N, lh, lw, 1), and for each (C, 2) array given the per-sample (N, 2) array.
 * srcfd_tiles_stitch_device: the stitch alone, of the samples [s0, s1) (multiples of C) of the tiler's grid: sample s is plane
 * Pointers of the three calls: dense float32 / int32 arrays, 4-byte aligned.  The cut reads and writes element by element.  The
 * stitch loads from y_dev and stores to out_dev V floats at a time and takes the narrower V itself when the two pointers share less
 * than 4 V bytes of alignment (never SRCFD_EINVAL): the plan's align_bytes below.
 * src_index_dev[s] of y_dev (int32 device array of N entries, indexed by s) or, with NULL, plane s - s0; y_dev holds y_rows planes
 * of hh x hw float32.  Only the tiles of [s0, s1) are written.  A tile whose index lies outside [0, y_rows) is left as it was.
 *
 * Overlapping tiles with blended seams (srcfd_tiled_plan_overlap, srcfd_tiler_create_overlap; overlap 0 on both axes is exactly the
 * tiler above).  Per axis, y shown, x alike and independent:
 *   overlap oy coarse cells, 0 <= oy, 2*oy <= lh (a point lies in at most two tiles per axis); with oy > 0 or ox > 0 both hh % lh
 *   and hw % lw must be 0, sy = hh / lh.  Coarse stride ly = lh - oy; the field has H = TY*ly + oy rows and tile ty takes coarse
 *   rows [ty*ly, ty*ly + lh).  Fine stride Sy = ly*sy, fine overlap Oy = oy*sy (hh = Sy + Oy); the output has H*sy = TY*Sy + Oy
 *   rows.  The sample order is unchanged.  Ramp: wy[j] = float32((j + 0.5) / Oy), j = 0 .. Oy-1, the division in float64 and
 *   rounded once, computed on the host and uploaded at create (the device never divides); strictly increasing, inside (0, 1).
 *   Output row R: t1 = min(R / Sy, TY-1), r1 = R - t1*Sy.  If t1 >= 1 and r1 < Oy the row is blended from tile t1-1 at row r1 + Sy
 *   (value a) and tile t1 at row r1 (value b) with w = wy[r1]; otherwise it is tile t1, row r1, copied.
 *   Blend: a + w*(b - a), three float32 operations, each rounded, no fused multiply-add: equal contributions come out exactly.
 *   Two axes: x first inside each contributing tile row (top = ax + wx*(bx - ax) in tile row t1-1, bottom likewise in t1), then
 *   out = top + wy*(bottom - top).  An axis with one source does no arithmetic: a pixel outside every overlap zone has its tile's
 *   bits.  The order matters: y first gives other bits at the corners.
 * srcfd_tiled_plan_overlap: the plan's keys, then "overlap":[oy,ox],"stride":[ly,lx],"field":[H,W],"out":[H*sy,W*sx],
 *   "blend":{"grid":G,"block":256,"blocks_per_row":B,"ramp":[Oy,Ox]}|null.  With an overlap "stitch" is null, "blend" is the one
 *   blending stitch (one lane per output pixel position, B workgroups per output row) and intermediate_bytes = N*hh*hw*4: a
 *   blended pixel may need tiles of different chunks, so every chunk predicts into its own planes of an intermediate that holds
 *   all N samples, and one stitch follows the last chunk.  Without one "blend" is null and the rest is srcfd_tiled_plan's.
 *   Further refusals: an overlap below 0 or above half the tile, an output side that is no multiple of the input side, an output
 *   side above INT_MAX, N*hh*hw beyond the 64-bit element offsets, a stitch of more workgroups than one launch takes.
 * On a handle of srcfd_tiler_create_overlap with an overlap, run, cut and set_stream work as documented above on the
 * (TY*ly + oy, TX*lx + ox, C) field and the (TY*Sy + Oy, TX*Sx + Ox, C) output; srcfd_tiles_stitch_device takes the whole range
 * only (s0 == 0, s1 == N; anything else is SRCFD_EINVAL: a blended stitch needs every tile), and a PIXEL with a contributing
 * index outside [0, y_rows) is left as it was. */
typedef struct srcfd_tiler srcfd_tiler;
int srcfd_tiled_plan(int lh, int lw, int in_channels, int hh, int hw, int out_channels, int tiles_y, int tiles_x, int channels,
                     int max_chunk, int model_chunk, int align_bytes, char* buf, size_t len);
int srcfd_tiled_plan_overlap(int lh, int lw, int in_channels, int hh, int hw, int out_channels, int tiles_y, int tiles_x, int channels,
                             int overlap_y, int overlap_x, int max_chunk, int model_chunk, int align_bytes, char* buf, size_t len);
int srcfd_tiler_create(srcfd_model* m, int tiles_y, int tiles_x, int channels, int max_chunk, srcfd_tiler** out);
int srcfd_tiler_create_overlap(srcfd_model* m, int tiles_y, int tiles_x, int channels, int overlap_y, int overlap_x, int max_chunk,
                               srcfd_tiler** out);
void srcfd_tiler_destroy(srcfd_tiler* t);
int srcfd_tiler_set_stream(srcfd_tiler* t, void* stream);
int srcfd_tiler_run(srcfd_tiler* t, const float* field_dev, const float* in_affine_dev, const float* out_affine_dev, float* out_dev,
                    int flags, int64_t* nonfinite_dev);
int srcfd_tiles_cut_device(srcfd_tiler* t, const float* field_dev, const float* in_affine_dev, const float* out_affine_dev,
                           float* x_dev, float* in_affine_n_dev, float* out_affine_n_dev);
int srcfd_tiles_stitch_device(srcfd_tiler* t, const float* y_dev, int64_t y_rows, const int32_t* src_index_dev, int s0, int s1,
                              float* out_dev);

/* ---- hand-off into the solver state ---------------------------------------------------------
 * Replaces the three transposed assignments `solver.Var[k, 1:-1, 1:-1] = ml_initial_fields[c].T` and the
 * ghost-cell pass `_apply_bc_wrapper(k)` that follow the SR call (PyCFD_ML_accelerated.py:936-943,
 * bfs_ml_accelerated.py:1211-1218): x holds the u, v, p samples of ONE field; Var is the solver's
 * float64 (3, nx+2, ny+2) host array and is written completely (corners 0, as in a fresh solver).
 * bc[k]: apply_bc_configured's arrays (PyCFD_ML_accelerated.py:118-146), order left, right, top,
 * bottom; type 0 = Dirichlet (ghost = 2*value - inner), 1 = Neumann (ghost = inner).  left_profile:
 * optional [ny] Dirichlet values that override the left boundary row by row (the BFS inlet/wall mix,
 * bfs_ml_accelerated.py:524-562).  r: optional resampler applied first (BFS), or NULL. */
typedef struct srcfd_solver_bc {
  int type[4];
  double value[4];
  const double* left_profile;
} srcfd_solver_bc;
int srcfd_predict_into_solver_state(srcfd_model* m, srcfd_resampler* r, const float* x, const float* in_affine,
                                    const float* out_affine, const srcfd_solver_bc bc[3], double* Var, int flags,
                                    int64_t* n_nonfinite);

/* ---- coarse-mesh solver (the producer of the SR call's input) ------------------------------------
 * Replaces, for the lid-driven cavity, `CFDSolver(mesh, fluid, settings, bc).solve()` as `run_coarse_simulation` uses it
 * (PyCFD_ML_accelerated.py:694-761; kernels :110-328, time loop :396-505): float64, host.  bc_type / bc_value are
 * apply_bc_configured's arrays per variable (u, v, p), order left, right, top, bottom; 0 = Dirichlet, 1 = Neumann
 * (`_get_bc_arrays`, :352-375).  var_out receives the solver state Var (3, nx+2, ny+2) including ghost cells; the
 * coarse fields the SR call takes are Var[k, 1:-1, 1:-1].T (:755-759).  Returns SRCFD_EINVAL with a message when the
 * residuals turn NaN / Inf (the reference raises ValueError, :487-492). */
#define SRCFD_SCHEME_QUICK 0
#define SRCFD_SCHEME_UPWIND 1
#define SRCFD_CASE_LDC 0
#define SRCFD_CASE_BFS 1
typedef struct srcfd_coarse_problem {
  int nx, ny;
  double lx, ly;
  double reynolds, rho, dt;
  int scheme;                /* SRCFD_SCHEME_* */
  int max_iterations;
  double tolerance[3];       /* convergence_criteria u, v, p on rms / dt */
  int bc_type[3][4];
  double bc_value[3][4];
  /* backward-facing step (bfs_ml_accelerated.py:471-673): SRCFD_CASE_BFS overrides the left boundary with a wall below
   * step_height and a parabolic inlet (bulk velocity Ub over channel_height) above it, and under-relaxes u, v, p with
   * relax[] after each solve.  SRCFD_CASE_LDC ignores these five fields. */
  int case_type;             /* SRCFD_CASE_* */
  double relax[3];
  double step_height, channel_height, bulk_velocity;
} srcfd_coarse_problem;
int srcfd_coarse_solve(const srcfd_coarse_problem* problem, double* var_out, int* iterations, double rms[3]);

/* ---- fine-mesh solver on the device (the solve the SR warm start is for) --------------------------
 * Replaces `CFDSolver(...)` + the injection + `solver.solve()` of `run_fine_simulation_with_ml_init` / `run_normal_simulation`
 * (PyCFD_ML_accelerated.py:882-966, 1126-1184; bfs_ml_accelerated.py:1140-1300): the loop of srcfd_coarse_solve for the same
 * srcfd_coarse_problem (same validation; max_iterations is ignored, run() takes its own), float64, resident on `device`.
 * Inner sweeps: momentum Jacobi, pressure red-black (colour (i+j)&1, colour 0 first) -- the one deliberate difference from the
 * host's serial sweeps; tests/fine_solver_spec.py restates the whole loop in numpy and the device reproduces it bit for bit. */
typedef struct srcfd_fine_solver srcfd_fine_solver;
int srcfd_fine_solver_create(const srcfd_coarse_problem* problem, int device, srcfd_fine_solver** out);
void srcfd_fine_solver_destroy(srcfd_fine_solver* s);
/* var NULL: `_initialize_fields` (zero fields, :377-390).  Otherwise the interior of var (3, nx+2, ny+2), host float64, is
 * taken (ghosts and corners start at 0).  Then the injection sequence of :940-953: BCs (BFS: with the inlet), Old = Var,
 * linear_interpolation.  Resets the iteration count. */
int srcfd_fine_solver_init(srcfd_fine_solver* s, const double* var);
/* SR of the u, v, p samples of one coarse field (x: (3, lr, lr, 1) float32) written straight into the solver's device Var, then
 * the priming of srcfd_fine_solver_init with the solver's own BCs (BFS: with the inlet).  No field crosses to the host.  This is
 * srcfd_fine_batch_init_from_prediction on a batch of one. */
int srcfd_fine_solver_init_from_prediction(srcfd_fine_solver* s, srcfd_model* m, srcfd_resampler* r, const float* x,
                                           const float* in_affine, const float* out_affine, int flags, int64_t* n_nonfinite);
/* srcfd_fine_batch_init_from_fields_device and srcfd_fine_batch_get_fields_device on the batch of one that a srcfd_fine_solver
 * is: fields_dev and out_dev are (3, h, w) and (3, ny, nx). */
int srcfd_fine_solver_init_from_fields_device(srcfd_fine_solver* s, srcfd_resampler* r, const void* fields_dev, int dtype, void* stream);
int srcfd_fine_solver_get_fields_device(srcfd_fine_solver* s, void* out_dev, int dtype, void* stream);
/* Up to max_iterations more outer iterations (none once converged).  *iterations = outer iterations since init; rms = the
 * last _convergence_check's residuals; history [history_len][3] receives rms at every iteration count divisible by 100 that
 * this call reaches, in order (residual_history, :418-421).  run(N) then run(M) equals run(N+M) bit for bit.  NaN / Inf in
 * the residuals: SRCFD_EINVAL with srcfd_coarse_solve's message (the reference raises ValueError). */
int srcfd_fine_solver_run(srcfd_fine_solver* s, int max_iterations, int* iterations, double rms[3], double* history, int history_len);
/* Copies Var (3, nx+2, ny+2) to host memory. */
int srcfd_fine_solver_get_state(srcfd_fine_solver* s, double* var);
/* counters: [0] momentum sweeps executed, [1] pressure sweeps executed (one red-black pair each), [2] device operations
 * enqueued (kernel launches, memsets), [3] host synchronisations; all since create.  last_sweeps: sweeps of the u, v and p
 * solves of the last outer iteration.  Either may be NULL. */
int srcfd_fine_solver_counters(const srcfd_fine_solver* s, int64_t counters[4], int last_sweeps[3]);
/* srcfd_fine_batch_set_mode on the batch of one that a srcfd_fine_solver is.  A resident run that meets NaN / Inf fails as
 * srcfd_fine_solver_run always does. */
int srcfd_fine_solver_set_mode(srcfd_fine_solver* s, int mode);

/* ---- batches of fine-mesh cases (the sweeps that make training data) ---------------------------------
 * Replaces the loop over Reynolds numbers of sr-simulation-data-creation.ipynb cell 2: n_cases problems with one nx, ny, scheme
 * and case_type (everything else may differ per case) advance together, the case index as the second grid dimension of every
 * launch (csrc/fine_solver.hip; a srcfd_fine_solver is a batch of one).  Each case computes what a srcfd_fine_solver of its own
 * computes, bit for bit, whatever the batch size and its position in it.  A case that converges, or whose residuals stop being
 * finite, is frozen; the others go on. */
typedef struct srcfd_fine_batch srcfd_fine_batch;
#define SRCFD_CASE_RUNNING 0   /* also: stopped only because run()'s iteration budget ended; resumable */
#define SRCFD_CASE_CONVERGED 1
#define SRCFD_CASE_DIVERGED 2
/* SRCFD_EINVAL, naming the case and the field, when a problem is invalid or differs from case 0 in nx, ny, scheme or
 * case_type, and when n_cases is outside 1..64. */
int srcfd_fine_batch_create(const srcfd_coarse_problem* problems, int n_cases, int device, srcfd_fine_batch** out);
void srcfd_fine_batch_destroy(srcfd_fine_batch* b);
/* var NULL: zero fields; otherwise (n_cases, 3, nx+2, ny+2) host float64, each case as srcfd_fine_solver_init takes its own.
 * Every case is RUNNING again, at iteration 0. */
int srcfd_fine_batch_init(srcfd_fine_batch* b, const double* var);
/* SR of n_warm coarse fields (x: (3*n_warm, lr, lr, 1) float32, u, v, p of each; affines (3*n_warm, 2) or NULL) written into
 * the device Var of the cases cases[0..n_warm) (NULL: n_warm == n_cases, case i takes field i); every other case starts from
 * zero fields, as srcfd_fine_batch_init(b, NULL) starts it.  Then the priming of srcfd_fine_batch_init: every case is live
 * again.  r: NULL, or the resampler from the model's output to the batch's mesh.  No field crosses to the host.
 * SRCFD_EINVAL: n_warm outside 1..n_cases, a case index out of range or listed twice, model and batch on different devices, a
 * prediction mesh that is not the batch's, a multi-channel model, a resampler that does not match the model.  n_nonfinite: the
 * NaN guard's count over all warm samples.  The network chooses its kernels by the sample count, so a warm case's initial
 * field has the bits of a 3*n_warm-sample prediction: they depend on n_warm (to f32 rounding), unlike everything the solver
 * computes from a given Var. */
int srcfd_fine_batch_init_from_prediction(srcfd_fine_batch* b, srcfd_model* m, srcfd_resampler* r, const float* x, int n_warm,
                                          const int* cases, const float* in_affine, const float* out_affine, int flags,
                                          int64_t* n_nonfinite);
/* srcfd_fine_batch_init_from_prediction without the network: fields that are already on the device -- a plainly interpolated
 * coarse field (the control arm of a warm-start study), a torch tensor, another batch's srcfd_fine_batch_get_fields_device.
 * fields_dev: (3*n_warm, h, w) of dtype SRCFD_F32 or SRCFD_F64, dense, aligned to its element; u, v, p of each field in the layout
 * of the SR prediction and the coarse-field files, field[j, i] -> Var[k, 1+i, 1+j].  r NULL: (h, w) is the batch's (ny, nx).
 * Otherwise (h, w) is the resampler's input, its output is the batch's (ny, nx), and the fields pass through it in float64
 * (srcfd_resample_device[_f64]'s products) into the resampler's own scratch, sized from n_warm; nothing else is allocated.  The
 * cases cases[0..n_warm) take the fields (NULL: case i takes field i, i < n_warm), every other case starts from zero fields, then
 * the priming of srcfd_fine_batch_init: every case is RUNNING at iteration 0.  Values are taken as they are -- no NaN guard, as
 * with a host var.  Ordering: the batch's own stream waits for everything enqueued on `stream` (a hipStream_t; NULL: the default
 * stream) up to the call, so the caller does not synchronise first; the call returns when the state is primed, as
 * srcfd_fine_batch_init does, and fields_dev is then no longer in use.  SRCFD_EINVAL, naming the argument: a dtype other than
 * the two, n_warm outside 1..n_cases, a case index out of range or listed twice, a resampler whose output is not the batch's mesh
 * or that lives on another device.  (The C side cannot see h and w of fields_dev; the Python binding checks them.)  Everything
 * is checked before anything is enqueued: a refused call leaves the batch as it was. */
int srcfd_fine_batch_init_from_fields_device(srcfd_fine_batch* b, srcfd_resampler* r, const void* fields_dev, int dtype, int n_warm,
                                             const int* cases, void* stream);
/* The inverse transposition: out_dev (3*n, ny, nx) of dtype SRCFD_F32 or SRCFD_F64, dense, aligned to its element, receives
 * out[3c+k, j, i] = Var[k, 1+i, 1+j] of the cases cases[0..n) (NULL: n == n_cases, all cases in order) -- the fields of
 * FineSolverBatch.fields(), without a host copy.  float64: an exact copy; float32: rounded to nearest.  Needs an initialised
 * batch.  Ordering: the batch's stream waits for `stream` (a hipStream_t) as above, the copy is complete when the call returns,
 * and `stream` is made to wait for it as well.  Counts one host synchronisation (counters[3]).  SRCFD_EINVAL as above. */
int srcfd_fine_batch_get_fields_device(srcfd_fine_batch* b, int n, const int* cases, void* out_dev, int dtype, void* stream);
/* Up to max_iterations more outer iterations of every case that is RUNNING; returns when none is, or when the budget is
 * spent.  Per case: iterations[n] (a frozen case keeps the count at which it froze), status[n] (SRCFD_CASE_*), rms[n][3] of
 * its last convergence check, history[n][history_len][3] = its rms at its iteration counts divisible by 100 that this call
 * reaches.  A diverged case is no error: the call returns SRCFD_OK and reports SRCFD_CASE_DIVERGED for it. */
int srcfd_fine_batch_run(srcfd_fine_batch* b, int max_iterations, int* iterations, int* status, double* rms, double* history,
                         int history_len);
/* Copies Var of case case_index (3, nx+2, ny+2), or of all cases (n_cases, 3, nx+2, ny+2) for -1, to host memory. */
int srcfd_fine_batch_get_state(srcfd_fine_batch* b, int case_index, double* var);
/* counters as srcfd_fine_solver_counters, with [0] and [1] counting per inner solve the sweeps of the live case that took the
 * most (the launches that did work); last_sweeps[n][3]: each case's own sweeps in its last outer iteration. */
int srcfd_fine_batch_counters(const srcfd_fine_batch* b, int64_t counters[4], int* last_sweeps);
/* ---- resident mode: small meshes, one workgroup per case, many outer iterations per launch ------------
 * SRCFD_FINE_MODE_LAUNCHES (the default) issues one launch per inner sweep, which is what a 400x400 mesh wants and what costs a
 * small mesh its whole solve.  SRCFD_FINE_MODE_RESIDENT gives every case one workgroup that runs the case's outer loop, inner
 * sweeps included, for up to 100 outer iterations per launch; the cases then advance at their own pace.  The state is the same
 * device state and the bits are the same bits (tests/fine_solver_spec.py), so the mode may change between any two run calls
 * and init, init_from_prediction, run and get_state work alike in both.  run() launches chunks that end at the next multiple of
 * 100 of the batch's iteration count or with the budget, with one launch, one status copy and one host synchronisation each.
 * Counters in resident mode: [2] and [3] count one launch and one synchronisation per chunk; [0] and [1] grow per chunk by the
 * largest momentum (u and v) and the largest pressure sweep total that a live case ran in it; last_sweeps is unchanged in
 * meaning.
 * srcfd_fine_resident_supported: 1 when a mesh can run resident, else 0 -- 3 <= nx, ny <= 64, the largest
 * mesh at which it measured faster than a launch per sweep.  Needs no device.
 * set_mode: SRCFD_EINVAL for an unknown mode and for RESIDENT on an unsupported mesh, with the mesh and the bound in the
 * message; the handle keeps its mode. */
#define SRCFD_FINE_MODE_LAUNCHES 0
#define SRCFD_FINE_MODE_RESIDENT 1
int srcfd_fine_resident_supported(int nx, int ny);
int srcfd_fine_batch_set_mode(srcfd_fine_batch* b, int mode);
/* Device bytes a batch allocates: n_cases x ((14 planes x (nx+2)(ny+2) + 9 nx) x 8 + one status block + one resident record +
 * one parameter block).  Needs no device. */
int srcfd_fine_batch_footprint(int nx, int ny, int n_cases, int64_t* device_bytes);
/* ---- direct pressure solve: four float64 matrix products in place of the red-black sweeps -------------
 * The inner pressure solve keeps the ghost ring frozen, so it is a Dirichlet 5-point Poisson problem on the nx x ny interior for
 * every case type and boundary condition, and the sine transform (DST-I) diagonalises it:
 *   p = Sx [ (Sx g Sy) / Lambda ] Sy,  g = rhs - the ghost neighbours' terms,  Lambda[a][b] = volp (lambda_x[a]/dx^2 + lambda_y[b]/dy^2).
 * SRCFD_PRESSURE_SWEEPS (the default) is the red-black solve with the launches and bits it always had.  SRCFD_PRESSURE_DIRECT
 * replaces it, in launch mode, by those four products on the f64 matrix cores (csrc/poisson_direct.hip): four launches and no
 * status read per pressure solve, the system solved to rounding where the sweeps stop at 1e-6 or at their cap of 1000.  Everything
 * around the solve is unchanged.  A case's bits still depend on neither the batch size nor its place in the batch, but there is no
 * numpy twin with equal bits: the mode is held by tolerance (tests/poisson_direct_ref.py).  It follows another trajectory to the
 * same fixed point as the sweeps.  A direct solve counts as 1 in counters[1] and in last_sweeps[.][2].
 * set_pressure_solver may be called between any two run calls.  The first switch to DIRECT allocates, per handle, the two bases
 * (padded to multiples of 32) and two nx x ny float64 planes per case; a handle that never switches allocates nothing more.
 * SRCFD_EINVAL, the handle unchanged: an unknown value; DIRECT on a handle in SRCFD_FINE_MODE_RESIDENT, and set_mode(RESIDENT) on a
 * DIRECT handle -- the resident mode has no direct path; the message names both settings.
 * srcfd_poisson_basis: S (n x n, row-major) and lambda (n) of one axis, either may be NULL -- S[a][b] = sqrt(2/(n+1)) sin(pi (a+1)(b+1)/(n+1)),
 * exactly symmetric, lambda[a] = -4 sin^2(pi (a+1) / (2 (n+1))), every entry evaluated in long double and rounded once.  Needs no
 * device.  SRCFD_EINVAL for n < 1. */
#define SRCFD_PRESSURE_SWEEPS 0
#define SRCFD_PRESSURE_DIRECT 1
int srcfd_fine_batch_set_pressure_solver(srcfd_fine_batch* b, int solver);
int srcfd_fine_solver_set_pressure_solver(srcfd_fine_solver* s, int solver);
int srcfd_poisson_basis(int n, double* S, double* lambda);

/* ---- training -----------------------------------------------------------
 * One optimisation step of SuperResolutionAE, split so that a data-parallel driver can put its
 * gradient all-reduce between the two halves (one flat f32 buffer per step).
 * Replaces `SuperResolutionAE.train_step` + `Adam()` (sr-ae-conv.ipynb:c306-320, c556).
 * Parameters, gradients and Adam moments are caller-owned flat f32 DEVICE arrays in Keras'
 * trainable_weights order (per layer: kernel then bias, Keras layouts); srcfd_trainer_get_params
 * returns the model's current values in that order (host). */
int srcfd_trainer_create(const srcfd_model* m, int max_batch, srcfd_trainer** out);
void srcfd_trainer_destroy(srcfd_trainer* t);
int64_t srcfd_trainer_num_params(const srcfd_trainer* t);
int srcfd_trainer_get_params(const srcfd_trainer* t, float* params_host);
/* Which training path create chose (read-only): *fused_tail = 1 when the last four layers run as the two fused launches
 * (tail32 forward, tail_bwd32 backward), *fused_encoder = 1 when the encoder's forward pass runs fused (train_enc); 0 = layer
 * by layer.  Either pointer may be NULL. */
int srcfd_trainer_get_plan(const srcfd_trainer* t, int* fused_tail, int* fused_encoder);
/* Forward + backward on n <= max_batch samples: x_dev (n,h,w,c) inputs, y_dev targets of the model's
 * output shape.  ADDS d/dparams of loss_scale * sum((pred - y)^2) into grads_dev (zero it first; pass
 * loss_scale = 1 / (global batch * output elements) for Keras' reduce_mean(mse)) and adds the local sum of
 * squared errors to *sse_dev (device double, may be NULL).  Enqueues on hip_stream, no synchronisation: part of the weight
 * gradients runs on a stream of the trainer's own that forks from and joins hip_stream inside the call.  From the second
 * call with the same params_dev / grads_dev / sse_dev / n / loss_scale the step is replayed as one hipGraph (x_dev and
 * y_dev are first copied to staging buffers, so they need not stay at one address).
 * Pointers: x_dev, y_dev dense (n, ...) float32, params_dev / grads_dev dense float32 of srcfd_trainer_num_params elements, all
 * 4-byte aligned; sse_dev 8-byte aligned.  The staging copy is one kernel of 16-byte accesses when x_dev and y_dev are both 16-byte
 * aligned and both element counts are multiples of 4, else two device-to-device copies (the narrower path, same bits); params_dev
 * is read and grads_dev written one element at a time through the trainer's index map.
 * One trainer, one stream at a time: the activations, gradient slabs, staging buffers and step graphs belong to the trainer, so
 * calls on the SAME trainer (this entry, the _ex one below) are ordered only when they are enqueued on the same stream; a caller
 * that changes streams between two calls orders them itself.  srcfd_adam_step keeps no state of its own: it is ordered by the
 * stream it is given, like any kernel on the caller's arrays. */
int srcfd_trainer_forward_backward(srcfd_trainer* t, const float* params_dev, const float* x_dev, const float* y_dev, int n,
                                   float loss_scale, float* grads_dev, double* sse_dev, void* hip_stream);
/* The same with flags.  SRCFD_TRAIN_OVERWRITE: grads_dev and *sse_dev are WRITTEN, not added into (every parameter's gradient is
 * stored by exactly one thread of the step's last launch): a step needs no zero-fill launches in front of it.  Without the flag
 * this is srcfd_trainer_forward_backward (accumulation over several calls, e.g. micro-batches of one optimiser step). */
#define SRCFD_TRAIN_OVERWRITE 1
/* SRCFD_TRAIN_SAME_PARAMS: params_dev holds exactly what it held at this trainer's previous forward_backward call (the second and
 * later micro-batches of one optimiser step): the per-call re-packing of the parameters into the kernels' operand layouts (one
 * 18 us launch) is skipped.  Wrong gradients, silently, if the parameters did change -- the caller's contract. */
#define SRCFD_TRAIN_SAME_PARAMS 2
int srcfd_trainer_forward_backward_ex(srcfd_trainer* t, const float* params_dev, const float* x_dev, const float* y_dev, int n,
                                      float loss_scale, float* grads_dev, double* sse_dev, int flags, void* hip_stream);
/* What the last successfully enqueued forward_backward call of this trainer ran with (read-only host state, no HIP call, no
 * stream; all zero before the first call): *n its samples; *tail_seg the segments per sample of the fused tail's forward launch,
 * *tail_blocks that launch's workgroups, *bwd_blocks the workgroups (= weight-gradient slabs) of the fused tail's backward launch,
 * all three 0 when the tail is not fused (srcfd_trainer_get_plan); *launch 0 for plain launches, 1 for the call that captured the
 * step graph and launched it, 2 for a replay of a captured graph.  A trainer holds at most 8 step graphs; calls with a further
 * key run as plain launches.  Any pointer may be NULL. */
int srcfd_trainer_last_step(const srcfd_trainer* t, int* n, int* tail_seg, int* tail_blocks, int* bwd_blocks, int* launch);
/* Keras Adam update, step counted from 1: alpha_t = lr*sqrt(1-beta2^t)/(1-beta1^t); p -= alpha_t*m/(sqrt(v)+eps).
 * Pointers: four dense float32 arrays of n elements, 4-byte aligned (one element per lane). */
int srcfd_adam_step(float* params_dev, const float* grads_dev, float* m_dev, float* v_dev, int64_t n, int step, float lr,
                    float beta1, float beta2, float eps, void* hip_stream);

#ifdef __cplusplus
}
#endif
#endif /* SRCFD_H */
