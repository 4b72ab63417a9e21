/*
 * se_engine.h - C ABI of the MI355X-native streaming speech-enhancement engine (libse_engine.so).
 *
 * The reference (KI-D/Speech-Enhancement-Mi) has no FFI: its plug-in point is the Python model class
 * (README.md:22).  This ABI is what a drop-in TemporalCRN class binds instead of running torch ops; each
 * entry point names the reference interface it replaces (file:line into the reference tree).  The
 * reference-side binding (ctypes) is shown in INTEGRATION.md and shipped in
 * speech_enhancement_mi_amd/crn.py.
 *
 * Conventions
 *  - plain C, no torch types.  All tensor pointers are DEVICE pointers (HIP, fp32, contiguous) unless
 *    a parameter says "host".  Pointers are borrowed for the duration of the call only.
 *  - every call enqueues on the caller's hipStream_t (passed as void*; NULL = default stream) and does
 *    not synchronise; the caller serialises calls per handle (the reference class is not re-entrant
 *    either, CRN.py:325-337).
 *  - return 0 on success, negative se_status on error; se_last_error() gives the message (the Python
 *    shim re-raises it as RuntimeError, mirroring the reference's exceptions-only convention).
 */
#ifndef SE_ENGINE_H
#define SE_ENGINE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SE_MAX_LEVELS 8

typedef enum {
    SE_OK = 0,
    SE_ERR_ARG = -1,        /* bad argument / unsupported configuration */
    SE_ERR_KEY = -2,        /* unknown checkpoint key */
    SE_ERR_SHAPE = -3,      /* parameter shape mismatch */
    SE_ERR_STATE = -4,      /* call order (step before reset, flag=True with another batch, ...) */
    SE_ERR_HIP = -5,        /* HIP runtime error */
    SE_ERR_PARAM_MISSING = -6 /* a weight was never loaded */
} se_status;

/* TemporalCRN.__init__ kwargs (CRN.py:415-417, config.yaml:205-217).  win/hop are in samples
 * (= round(sample_rate/1000 * win_length_ms), the speechbrain STFT convention, CRN.py:421-425). */
typedef struct {
    int32_t num_levels;                 /* len(num_channels) */
    int32_t channels[SE_MAX_LEVELS];    /* num_channels */
    int32_t num_freqs;                  /* n_fft/2+1 */
    int32_t hidden;
    int32_t num_layers;                 /* GRU layers */
    int32_t num_inputs;                 /* microphones M */
    int32_t kernel_size;                /* 3 */
    int32_t n_fft, win, hop;
    int32_t segment_length;             /* K = 3200 */
    int32_t variant;                    /* 0 = CRN.py TemporalCRN (ReLU); 1 = CRN_ELU.py TemporalCRN (ELU, gated 1x1 convs,
                                           three 5x5 frequency-dilated preconv blocks, atan2 phase; CRN_ELU.py:321-365);
                                           2 = distillation_crn.py TemporalCRN, the student architecture (as 1, but arctan
                                           phase and gLN denominator sqrt(var)+eps; distillation_crn.py:51,340) */
    int32_t precision;                  /* 0 = fp32-accurate contractions (6-term split-bf16 MFMA); 1 = fp16 MFMA operands with
                                           fp32 accumulation for the convolutions and dense layers (`model.half()`; OUTSIDE the
                                           1e-4 parity bar: 2e-3 relative); 2 = 3-term split-bf16 (hi*hi + hi*mid + mid*hi, 16
                                           mantissa bits per operand, fp32 accumulation: inside the 1e-4 / 0.02 dB bar, half the
                                           matrix work of mode 0; the fast mode of BASELINE config 5).  The recurrence stays fp32. */
} se_config;

typedef struct se_engine se_engine;

/* TemporalCRN(**config['TemporalCRN'])  (CRN.py:415-451; train.py:58, predict.py:45) */
int se_create(const se_config *cfg, int device, se_engine **out);
void se_destroy(se_engine *e);
/* message of the last failing call on this handle (or of se_create when e == NULL) */
const char *se_last_error(const se_engine *e);

/* load_state_dict(): one tensor per call, by reference checkpoint key (e.g.
 * "convlist.0.conv.weight", "gru.sequence_model.weight_hh_l1").  `data` is a HOST pointer.
 * The `net.0.*` aliases the reference's state_dict carries (CRN.py:314-316) are accepted. */
int se_load_param(se_engine *e, const char *key, const float *host_data, const int64_t *shape, int ndim);

/* TemporalCRN.reset() + lazy state allocation for B streams (CRN.py:498-503, 325-326). */
int se_reset(se_engine *e, int batch);

/* Reset ONE stream of the batch (a call ends, a new caller takes its slot) while the others keep their state: zeroes that
 * stream's conv time buffers and GRU state, i.e. what TemporalCRN.reset() does (CRN.py:498-503) restricted to row
 * `stream_index` of every state tensor.  The reference can only reset the whole batch; this is the continuation API a
 * server needs around the path.  Enqueued on `stream`. */
int se_reset_stream(se_engine *e, int stream_index, void *stream);

/* One hot-path step: all B streams advance by one K-sample window.
 * wav_in [B, M, K] -> wav_out [B, K]  == istft_trans(forward(stft_trans(x)))  (CRN.py:505-520, 454-496) */
int se_step(se_engine *e, const float *wav_in, float *wav_out, void *stream);

/* TemporalCRN.realtime_process(mixture, flag) (CRN.py:560-589): mixture [B, M, L] -> out [B, L].
 * flag == 0: reset + K/2 left pad (stripped again); flag != 0: carry state, B must match. */
int se_realtime_process(se_engine *e, const float *mixture, int batch, int64_t length, int flag,
                        float *out, void *stream);

/* Ragged batch (the reference's utterances are 1 .. 3.75 s long, data_c.py:155-173): stream b holds lengths[b] <= max_length valid
 * samples of mixture [B, M, max_length]; every stream gets exactly the output it would get alone - its own zero padding (samples past
 * its length read as zeros) and out[b, lengths[b]:] = 0.  lengths is a HOST array.
 * This is se_realtime_process_chains (below) with the one flag for every stream, and everything said there holds: a stream that ends
 * before the longest one keeps its own continuation state, and when the segment counts are NON-INCREASING (sort the batch; the Python
 * shim does) every segment is launched for the prefix of streams that still take part in it only - every layout is stream-major, so
 * nothing moves; grids, GEMM rows and recurrence rows shrink (plane path, CRN.py variant, batches on the plane-GEMM route;
 * SE_RAGGED_COMPACT=0 turns it off).  With unsorted counts every stream runs every segment. */
int se_realtime_process_ragged(se_engine *e, const float *mixture, int batch, int64_t max_length, const int64_t *lengths_host, int flag, float *out,
                               void *stream);

/* A batch of chunk CHAINS (the reference continues every stream of its chunk chain, CRN.py:568-575, data_c.py:60-84, 155-173): B callers,
 * each with its own chunk length and its own flag, in one call.  lengths and flags are HOST arrays of `batch` entries.
 *  - stream b is mixture[b, :, :lengths[b]] and ZERO beyond, whatever the padding holds; 0 < lengths[b] <= max_length.
 *  - flags[b] == 0: stream b starts from zero state, gets the K/2 left pad and has it stripped again (first segment at -K);
 *    flags[b] != 0: it continues row b of the carried state, no pad (first segment at -K/2).
 *  - a call with any flag set needs a carried batch of the same size (SE_ERR_STATE otherwise); with all flags zero the batch size may
 *    change, like flag = 0 of se_realtime_process.
 *  - out[b, lengths[b]:] = 0.
 *  - afterwards the state of EVERY stream (conv time buffers of every encoder level, the preconv buffers of variants 1 / 2, GRU h of
 *    every layer) is what that stream alone would carry after its own last segment: the state se_export_state, se_step,
 *    se_reset_stream and a following se_realtime_process* call see.  A chains call with a new caller's flag at 0 therefore replaces
 *    se_reset_stream + se_realtime_process_ragged, and no stream has to wait for the longest one.
 * Every stream keeps the segment geometry it has alone (utility.py:327-329, 360-368 with lead = flags[b] ? 0 : K/2); the call runs
 * max_b N_b segments.  The state of a stream is saved when its last segment has passed a stage (encoder rows on the encoder's stream,
 * layer l's h after layer l) and written back when the call ends; a reset among continuing streams zeroes that stream's rows at
 * entry.  Prefix compaction (see se_realtime_process_ragged) when the segment counts N_b are non-increasing.  A uniform batch (equal
 * flags, every length == max_length) is exactly se_realtime_process: no save, no restore, no extra launch. */
int se_realtime_process_chains(se_engine *e, const float *mixture, int batch, int64_t max_length, const int64_t *lengths_host,
                               const uint8_t *flags_host, float *out, void *stream);

/* The segment geometry both engines give a stream of `length` samples cut into half-overlapping segments of segment_length: *nseg
 * segments, the first starting at sample *off0 of the stream (-K/2 when it continues, -K after a reset, whose K/2 lead of zeros the
 * overlap average strips again: *skip).  Host arithmetic only, no device, no engine: what every *_realtime_process* call computes per
 * stream, exported so that a binding's own copy (engine.chain_geometry) can be checked against it.  SE_ERR_ARG on a non-positive
 * size or a null pointer. */
int se_chunk_geometry(int segment_length, int64_t length, int continues, int64_t *nseg, int64_t *off0, int64_t *skip);

/* Per-stage entry points (parity tests; same arithmetic as inside se_step).
 * se_stft:    stft_trans  (CRN.py:505-512): seg [n, K] -> spec [n, F, T, 2]   (n = B*M rows)
 * se_istft:   istft_trans (CRN.py:514-520): spec [n, F, T, 2] -> wav [n, K]
 * se_forward: TemporalCRN.forward (CRN.py:454-496): x [B, M, F, T, 2] -> y [B, F, T, 2]; stateful. */
int se_stft(se_engine *e, const float *seg, int n, float *spec, void *stream);
int se_istft(se_engine *e, const float *spec, int n, float *wav, void *stream);
int se_forward(se_engine *e, const float *x, float *y, void *stream);

/* Debug taps of the last forward, converted to the reference's [B, C, F, T] layout, copied to HOST.
 * name: "feat" (encoder input, after the preconv blocks for variants 1/2), "enc0".."encN", "gru", "dec0".."decN";
 * "ft0".."ftL": the pre-activation feature maps the distillation student returns (distillation_crn.py:467-477): last encoder
 * convolution [B, C, F, T], fc_output_layer output ([B, T, D] memory), transposed-convolution outputs of decoder blocks 0..L-2.
 * Synchronises the stream.  *count = elements. */
int se_read_tap(se_engine *e, const char *name, float *host_out, int64_t capacity, int64_t *count, void *stream);
/* The student's distillation feature maps "ft0".."ft<L>" (distillation_crn.py:467-477: last encoder convolution, fc layer, transposed
 * convolutions, all before their activation) written to DEVICE memory as [B, C, F, T] fp32 on `stream`; no host copy.  Other tap names:
 * SE_ERR_KEY (host-only debugging taps). */
int se_read_tap_dev(se_engine *e, const char *name, float *dev_out, int64_t capacity, int64_t *count, void *stream);

/* Streaming state hand-over: encoder time buffers "buf<i>" [B, Cin, F, 2d] and GRU
 * hidden "h" [layers, B, H] in the reference's layouts, HOST pointers; variants 1/2 add the preconv buffers
 * "pbuf<i>" [B, 2M-1, F, 4].  Synchronises. */
int se_export_state(se_engine *e, const char *name, float *host_out, int64_t capacity, int64_t *count, void *stream);
int se_import_state(se_engine *e, const char *name, const float *host_in, int64_t count, void *stream);

/* Introspection: algorithmic FLOPs per frame (dense contractions only) and geometry. */
double se_flops_per_frame(const se_engine *e);
int se_frames_per_segment(const se_engine *e); /* T */

/* Per-kernel timing for bench.py's roofline leg: with profiling enabled every kernel launch is bracketed by
 * two HIP events on the launch stream.  se_profile(e, on) clears the counters; se_profile_read() folds the
 * pending events (synchronises) and returns entry `index` (kernel function name, launch-site label, total
 * milliseconds, launches, algorithmic FLOPs per launch); returns 1 past the last entry. */
int se_profile(se_engine *e, int enable);
int se_profile_read(se_engine *e, int index, char *kernel, char *label, int cap, double *ms_total,
                    int64_t *launches, double *flops_per_launch);

int se_abi_version(void);  /* 5: the first-generation training entry points are gone (se_train_conv_w, se_train_conv_wgrad_det and
                              se_train_gemm_tn_det are the only convolution / weight-gradient forms);
                              4 since round 3 (fsn_config.precision, se_sig_*, fused training stages, se_realtime_process_ragged, se_read_tap_dev, se_loss_stoi_*);
                              additions at 4: fsn_train_ws_bytes, fsn_train_fwd, fsn_train_bwd; se_train_add_csum, se_distill_*, se_gbf_* (forward and backward);
                              additions at 5: se_realtime_process_chains; fsn_realtime_process_chains, fsn_reset_stream, fsn_export_state,
                              fsn_import_state; se_chunk_geometry; fsn_train_ws_bytes_chains, fsn_train_fwd_chains, fsn_train_bwd_chains; se_gtsa_* (GTSA inference); se_hifi_* (HiFi-GAN generator inference, and its training: se_hifi_lstm_train_fwd, se_hifi_*_bwd, se_hifi_chansum); se_loss_pesq_* (the perceptual term of GTSA.compute_loss) */
/* sizeof(se_config) / sizeof(fsn_config) as this library was built: a binding checks its own struct mirror against these
 * before the first se_create (a short struct would leave `precision` reading whatever follows it). */
int se_config_size(void);
int fsn_config_size(void);

/* ---- FullSubNet (reference fullsubnet.py:685-961; BASELINE config 3) -------------------
 * Same conventions as the se_* calls above.  Checkpoint keys: fb_model.* / sb_model.* of FullSubNet.state_dict(). */
typedef struct {
    int32_t num_freqs, num_mics;
    int32_t fb_hidden, sb_hidden;       /* fb_model_hidden_size, sb_model_hidden_size */
    int32_t num_layers;
    int32_t sb_neighbors, fb_neighbors; /* sb_num_neighbors (15), fb_num_neighbors (0: the only supported value) */
    int32_t look_ahead;                 /* 0 */
    int32_t n_fft, win, hop, segment_length;
    int32_t precision;                  /* ABI 4: 0 = fp32-accurate LSTM contractions (6-term split-bf16 MFMA); 2 = 3-term split-bf16
                                           ("bf16x3": inside the 1e-4 / 0.02 dB parity bar, half the matrix work); 1 is not offered */
} fsn_config;

typedef struct fsn_engine fsn_engine;

/* FullSubNet(**config['FullSubNet'])  (fullsubnet.py:686-767; config.yaml:153-172; LSTM, ReLU / no output activation) */
int fsn_create(const fsn_config *cfg, int device, fsn_engine **out);
void fsn_destroy(fsn_engine *e);
const char *fsn_last_error(const fsn_engine *e);
int fsn_load_param(fsn_engine *e, const char *key, const float *host_data, const int64_t *shape, int ndim);
/* reset_state (fullsubnet.py:826-832): zero LSTM states, reset both CumLayerNorm running means */
int fsn_reset(fsn_engine *e, int batch);
/* FullSubNet.forward (fullsubnet.py:769-824): x [B, 2M, F, T] (re x M, then im x M) -> compressed mask [B, 2, F, T]; stateful */
int fsn_forward(fsn_engine *e, const float *x, float *crm, void *stream);
/* FullSubNet.realtime_process(mixture, source, flag, train=False)[0] (fullsubnet.py:903-961): [B, M, L] -> [B, L] */
int fsn_realtime_process(fsn_engine *e, const float *mixture, int batch, int64_t length, int flag, float *out, void *stream);
/* A batch of chunk CHAINS, the contract of se_realtime_process_chains word for word, applied to realtime_process(train=False): B callers,
 * each with its own chunk length and its own flag, in one call.  lengths and flags are HOST arrays of `batch` entries.
 *  - stream b is mixture[b, :, :lengths[b]] and ZERO beyond, whatever the padding holds; 0 < lengths[b] <= max_length.
 *  - flags[b] == 0: stream b starts from zero LSTM state and reset norms, gets the K/2 left pad and has it stripped again;
 *    flags[b] != 0: it continues row b of the carried state, no pad.
 *  - a call with any flag set needs a carried batch of the same size (SE_ERR_STATE otherwise); with all flags zero the batch size may
 *    change.  A failing call leaves the engine usable.
 *  - out[b, lengths[b]:] = 0.
 *  - afterwards the state of EVERY stream (full-band h, c of every layer; sub-band h, c of every layer, the stream's F rows; both
 *    CumLayerNorm running means and both step counters, which are per stream) is what that stream alone carries after its own last
 *    window: the state a following fsn_realtime_process*, fsn_forward, fsn_reset_stream and fsn_export_state see.
 * Every stream keeps the window geometry it has alone (lead = flags[b] ? 0 : K/2); the call runs max_b N_b windows.  A stream's
 * full-band rows, mean and counter are saved right after the full-band stage of its last window (on the engine's side stream, which
 * runs one window ahead), its sub-band rows after the sub-band stage, and written back when the call ends; a reset among continuing
 * streams zeroes that stream's rows and counters at entry.  Prefix compaction when the window counts N_b are NON-INCREASING (sort a
 * fresh batch; the Python shim does): every window is launched for the streams still running only.  With unsorted counts every stream
 * runs every window.  A uniform batch (equal flags, every length == max_length) is exactly fsn_realtime_process: same launches, no
 * save, no restore. */
int fsn_realtime_process_chains(fsn_engine *e, const float *mixture, int batch, int64_t max_length, const int64_t *lengths_host,
                                const uint8_t *flags_host, float *out, void *stream);
/* reset_state + both CumLayerNorm.reset() (fullsubnet.py:826-832, 203-205) for ONE stream of the carried batch; the others keep streaming */
int fsn_reset_stream(fsn_engine *e, int stream_index, void *stream);
/* Streaming state hand-over in the reference's layouts, HOST pointers; synchronises.  Names: "fh", "fc" [layers, B, H_fb]; "sh", "sc"
 * [layers, B*F, H_sb], row b*F + f (fullsubnet.py:810-811, 829); "mean_fb", "mean_sb" [B]; "step_fb", "step_sb" [B]: the CumLayerNorm
 * step counters, small integers (0 .. 80) held exactly as floats, 0 = no mean yet.  Unknown name: SE_ERR_KEY; wrong count: SE_ERR_SHAPE. */
int fsn_export_state(fsn_engine *e, const char *name, float *host_out, int64_t capacity, int64_t *count, void *stream);
int fsn_import_state(fsn_engine *e, const char *name, const float *host_in, int64_t count, void *stream);
/* host copies of "fb_out" [B*T, F], "mean_fb" [B], "mean_sb" [B] after the last forward */
int fsn_read_tap(fsn_engine *e, const char *name, float *host_out, int64_t capacity, int64_t *count, void *stream);
double fsn_flops_per_frame(const fsn_engine *e);
/* Training (train_fullsubnet.py:137-145: autograd over realtime_process(train=False), fullsubnet.py:903-961).  All pointers are DEVICE
 * pointers; the calls enqueue on `stream`.  nseg = N windows of the chunk.
 * fsn_train_ws_bytes: workspace size for (batch, nseg): the activations of every LSTM step (gates, c, h) of all windows, laid out
 *   [T][N * rows][.] so that step t of every window is one slab, plus the backward's scratch (about 31 GB at 8 utterances x 3 s).
 * fsn_train_fwd: spec = se_sig_stft of the chunk [nseg][batch * M][T][F][2]; runs the windows in the engine's own order (CumLayerNorm
 *   updates, full band, unfold, sub band; fullsubnet.py:769-824), carries the state like fsn_realtime_process (flag = 0 resets it,
 *   fullsubnet.py:912-915), writes crm_out [nseg][batch][2][F][T] (pred_crm) and saves what the backward needs into ws.
 * fsn_train_bwd: dcrm [nseg][batch][2][F][T] = d loss / d crm of the same (batch, nseg, ws) -> the gradient of every fb_model.* /
 *   sb_model.* parameter in checkpoint layout, grads[] in state_dict order: per model (fb, then sb) weight_ih_l, weight_hh_l, bias_ih_l,
 *   bias_hh_l of each layer, then fc_output_layer.weight, fc_output_layer.bias; ngrads = 2 (4 num_layers + 2).  The BPTT stops at
 *   every window seam (the state is detached, fullsubnet.py:819-820) and the CumLayerNorm means are detached (fullsubnet.py:200).
 *   Deterministic: no float atomics, identical gradients run to run. */
int64_t fsn_train_ws_bytes(fsn_engine *e, int batch, int nseg);
int fsn_train_fwd(fsn_engine *e, const float *spec, int batch, int nseg, int flag, void *ws, float *crm_out, void *stream);
int fsn_train_bwd(fsn_engine *e, const float *dcrm, int batch, int nseg, void *ws, float *const *grads, int ngrads, void *stream);
/* Training over a batch of chunk CHAINS: the contract of fsn_realtime_process_chains (per-stream lengths and flags, HOST arrays of
 * `batch` entries; the same validation, error codes and texts; every stream leaves the state it alone would carry), applied to the
 * training forward and backward.  All three calls take the same (batch, max_length, lengths, flags) and derive the same plan from
 * them; the backward rebuilds it from these host arguments, and finds the device row table where the forward left it, in a header
 * region of ws.  nseg = N = max_b N_b windows (se_chunk_geometry per stream).
 *  - spec = se_sig_stft_rows of the chunk [N][batch * M][T][F][2] (per-row offset and length; a stream's windows past its own last
 *    one are all-zero spectra); crm_out and dcrm are dense [N][batch][2][F][T]; windows n >= N_b of stream b hold exact zeros in crm_out.
 *  - PACKED workspace when the window counts N_b are non-increasing (sort a fresh batch; the Python shim does): window n runs for the
 *    bact(n) streams still running and its activations go to packed rows base[n] = sum_{m<n} bact(m), so the workspace, the LSTM steps,
 *    the BPTT and the weight-gradient rows cover sum_b N_b windows, not N * batch.  The window seams are detached (fullsubnet.py:819-820,
 *    200), which is what makes the windows independent rows of the backward.  Otherwise (a carried batch keeps its slots) the dense
 *    layout of fsn_train_fwd: every stream runs every window, dead windows read zeros and their rows are restored afterwards.
 *  - a uniform batch (equal flags, every length == max_length) IS fsn_train_ws_bytes / fsn_train_fwd / fsn_train_bwd: same launches.
 *  - fsn_train_fwd_chains synchronises `stream` once, after uploading the plan (the host arrays live for the call only).
 * Deterministic like fsn_train_bwd.  fsn_train_ws_bytes_chains returns a negative SE_ERR_* code on a refused plan. */
int64_t fsn_train_ws_bytes_chains(fsn_engine *e, int batch, int64_t max_length, const int64_t *lengths_host, const uint8_t *flags_host);
int fsn_train_fwd_chains(fsn_engine *e, const float *spec, int batch, int64_t max_length, const int64_t *lengths_host, const uint8_t *flags_host,
                         void *ws, float *crm_out, void *stream);
int fsn_train_bwd_chains(fsn_engine *e, const float *dcrm, int batch, int64_t max_length, const int64_t *lengths_host, const uint8_t *flags_host,
                         void *ws, float *const *grads, int ngrads, void *stream);

/* ---- training loss (reference CRN.py:593-617 compute_loss) ------------------------------------------------
 * SI-SNR term, utility.cal_si_snr (utility.py:207-223), device-resident: separated / source [B, L] fp32 device tensors,
 * lens [B] int64 device tensor (samples that count per utterance).  fwd writes the per-utterance SI-SNR in dB to per_utt [B]
 * and 8 doubles of saved scalars per utterance to stats; bwd writes grad [B, L] = gscale[0] * d SI-SNR_b / d separated
 * (gscale is a 1-element device tensor: upstream gradient / B for the batch mean).  Enqueued on `stream`, no sync. */
int se_loss_sisnr_fwd(const float *separated, const float *source, const int64_t *lens, int batch, int64_t length, float *per_utt,
                      double *stats, void *stream);
/* STOI term of compute_loss (utility.stoi_loss, utility.py:821-916) as kernels, forward and backward w.r.t. the prediction.
 * Tables (device memory, built by the caller once: losses._plan): rs_w [5][W] + rs_first [5] = the 16 kHz -> 10 kHz polyphase filter
 * (Kaldi LinearResample, augment.py:478-545), hann_sym [256] = np.hanning(256) (utility.py:522), hann_per [256] = periodic Hann of the
 * spectrogram, band_lo / band_hi [15] = third-octave band bin ranges (utility.thirdoct, utility.py:480-518).  ws = se_loss_stoi_ws_floats
 * floats of scratch that carry the forward's intermediates to the backward.  D [batch] = STOI per utterance (0.99 for utterances too
 * short to score, utility.py:877-880); gD = d loss / d D; dpred [batch][length]. */
int64_t se_loss_stoi_ws_floats(int batch, int64_t length);
int se_loss_stoi_fwd(const float *clean, const float *pred, const int64_t *lens, int batch, int64_t length, const float *rs_w, const int *rs_first, int W,
                     const float *hann_sym, const float *hann_per, const int *band_lo, const int *band_hi, float *ws, float *D, void *stream);
int se_loss_stoi_bwd(const float *gD, const int64_t *lens, int batch, int64_t length, const float *rs_w, const int *rs_first, int W, const float *hann_sym,
                     const float *hann_per, const int *band_lo, const int *band_hi, float *ws, float *dpred, void *stream);
const char *se_loss_stoi_last_error(void);
/* Perceptual term of GTSA.compute_loss (utility.pesq_loss, utility.py:615-814; GTSA.py:411-433) as kernels, forward and backward w.r.t.
 * the prediction.  Row b is scored on its first lens[b] samples alone (reflect padding at its own end); a row of fewer than 20
 * spectrogram frames (lens[b] < 4864) gets a NaN value and a zero gradient.  Tables (device memory, built by the caller once:
 * losses._pesq_plan): win [512] = periodic Hann of Spectrogram(1024, 512, 256) (utility.py:727), edges [50] = Bark band bin edges
 * (bark2hz, utility.py:639-648), band_of [513] = bin -> band or -1, band_tab [5][49] = power density correction * Sp, absolute threshold
 * * 1e4, Zwicker exponent, (2 * threshold) ** exponent, band width in Bark (utility.py:653-710, 745, 772).  ws = se_loss_pesq_ws_floats
 * floats of scratch that carry the forward's intermediates to the backward.  value [batch] = -(4.5 - 0.1 sres - 0.0309 asres)
 * (utility.py:813-814); gvalue = d loss / d value; dpred [batch][length].  length >= 4864 and at most 896 frames (14.3 s). */
int64_t se_loss_pesq_ws_floats(int batch, int64_t length);
int se_loss_pesq_fwd(const float *clean, const float *pred, const int64_t *lens, int batch, int64_t length, const float *win, const int *edges,
                     const float *band_tab, float *ws, float *value, void *stream);
int se_loss_pesq_bwd(const float *gvalue, const int64_t *lens, int batch, int64_t length, const float *win, const int *band_of, const float *band_tab, float *ws,
                     float *dpred, void *stream);
const char *se_loss_pesq_last_error(void);
int se_loss_sisnr_bwd(const float *separated, const float *source, const int64_t *lens, int batch, int64_t length, const double *stats,
                      const float *gscale, float *grad, void *stream);

/* ---- training-step building blocks (reference train.py:195-204 = torch autograd over CRN.py:290-401, 196-287) --
 * fp32-exact MFMA kernels on device tensors; activations are [B][C][T][F] (F innermost).  speech_enhancement_mi_amd/train_ops.py is
 * the one launch layer over them (train_stages.py builds the models' passes on it); torch autograd is the checker.  The convolutions
 * and the weight gradients are se_train_conv_w, se_train_conv_wgrad_det and se_train_gemm_tn_det further down: weight gradients are
 * partial tiles per row split folded in a fixed order, the only form there is (no float atomics).
 * All calls enqueue on `stream` and return 0 or a negative se_status; se_train_last_error() gives the message. */
const char *se_train_last_error(void);
/* C[M][N] = act(A[M][K] W[N][K]^T + bias[N])  (act: 0 none, 1 ReLU, 2 ELU); bias may be NULL; K % 8 == 0 */
int se_train_gemm(const float *A, const float *W, const float *bias, float *C, int M, int N, int K, int act, void *stream);
/* all T steps of one GRU layer (CRN.py:269 nn.GRU) in one call, one launch per step: forward (r, z, n, gh_n saved per row in `gates`)
 * and the BPTT sweep with the gradient cut at segment
 * boundaries ((t + 1) % seg_len == 0: the carried state is detached per segment, CRN.py:281).  gi [B][T][3H], out [B][T][H],
 * gates [B][T][4H], whh_t = W_hh^T [H][3H]; scratch: 2 B H floats (forward), 4 B H floats (backward); backward: B <= 16 */
int se_train_gru_seq_fwd(const float *gi, const float *h0, const float *whh, const float *bhh, float *out, float *gates, float *hT, float *scratch,
                         int B, int T, int H, void *stream);
int se_train_gru_seq_bwd(const float *dout, const float *dhT, const float *gates, const float *out, const float *h0, const float *whh_t, float *dgi,
                         float *dgh, float *scratch, int B, int T, int H, int seg_len, void *stream);

/* ONE persistent launch per GRU layer and direction (csrc/gru_pseq.hip.h): H/16 resident workgroups per group of <= 32 streams keep
 * their W_hh slice in registers and exchange the state vector per step through write-through stores + an agent-scope arrival counter.
 * Replaces T dependent step launches (round 2).  Any number of streams: more than 32 run as independent 16-stream groups of the same
 * launch (rows must then be [B][T], ldN = 0) - which is how the training backward runs, because the state is detached at every segment
 * seam (CRN.py:281): S = segments x utterances independent streams of Tseg steps.  Rows of gi / out / gates / dout / dgi / dgh are
 * addressed as row(b, s) = (s / Tseg) * ldN + b * ldB + s % Tseg, which covers [B][T] (Tseg = T, ldN = 0, ldB = T) and the training
 * forward's segment-major [N][B][Tseg] (ldN = B * Tseg, ldB = Tseg).  scratch: se_train_gru_pseq_scratch_floats(B, H) floats; word [1]
 * of scratch is non-zero after a bounded-spin timeout (results invalid).  gates may be NULL in the forward (inference / no_grad).
 * seg_len as in se_train_gru_seq_bwd. */
int se_train_gru_pseq_scratch_floats(int B, int H);
int se_train_gru_pseq_supported(int B, int H);
int se_train_gru_pseq_fwd(const float *gi, const float *h0, const float *whh, const float *bhh, float *out, float *gates, float *hT,
                          float *scratch, int B, int T, int H, int Tseg, int64_t ldN, int64_t ldB, void *stream);
int se_train_gru_pseq_bwd(const float *dout, const float *dhT, const float *gates, const float *out, const float *h0, const float *whh_t,
                          float *dgi, float *dgh, float *scratch, int B, int T, int H, int Tseg, int64_t ldN, int64_t ldB, int seg_len,
                          void *stream);
/* The same two launches with a step count per stream (chunk chains: utterances of different lengths in one call).  steps: DEVICE int32
 * [B], 0 <= steps[b] <= T (clamped).  A group of streams runs max steps[b] dependent steps instead of T.  Stream b computes, bit for
 * bit, what the plain call gives for it alone with T = steps[b]: out / gates (dgi / dgh) rows s < steps[b], hT[b] after its own last
 * step (h0[b] where steps[b] = 0), dhT[b] entering at step steps[b] - 1.  Rows s >= steps[b] of out / gates / dgi / dgh are written as
 * zeros by the kernel; dout / gates / out are not read there. */
int se_train_gru_pseq_fwd_rows(const float *gi, const float *h0, const float *whh, const float *bhh, float *out, float *gates, float *hT,
                               float *scratch, int B, int T, int H, int Tseg, int64_t ldN, int64_t ldB, const int32_t *steps, void *stream);
int se_train_gru_pseq_bwd_rows(const float *dout, const float *dhT, const float *gates, const float *out, const float *h0, const float *whh_t,
                               float *dgi, float *dgh, float *scratch, int B, int T, int H, int Tseg, int64_t ldN, int64_t ldB, int seg_len,
                               const int32_t *steps, void *stream);

/* ---- round 3: the norm / pointwise / signal stages of the training step, forward and backward (csrc/train_fused.hip.h) ----
 * Layout: activations [S][C][T][F] fp32, S = N segments x B utterances, SEGMENT-major (stream n * B + b), so the time history of
 * segment n is the same tensor one slab (B streams) earlier and the per-segment loop of realtime_process (CRN.py:577-586) becomes one
 * launch per layer.  All gradients of per-channel parameters are produced as [S][C] slabs and folded by se_train_colsum: the
 * training step contains no float atomics (bit-reproducible gradients). */
typedef struct se_sig se_sig;   /* STFT tables: hamming(win) centred in n_fft, twiddles, overlap-add envelope */
int se_sig_create(int n_fft, int win, int hop, int segment_length, int device, se_sig **out);
void se_sig_destroy(se_sig *g);
/* stft_trans of ALL segments (CRN.py:505-512 + utility.padding / segmentation, utility.py:312-370): wav [B][M][L]; segment y of row
 * (b, m) covers samples off0 + y * seg_off + [0, K) (zero outside [0, L)) -> spec [nseg][B*M][T][F][2] */
int se_sig_stft(se_sig *g, const float *wav, int B, int M, int64_t L, int64_t off0, int64_t seg_off, int nseg, float *spec, void *stream);
/* istft_trans (CRN.py:514-520): spec [rows][T][F][2] -> wav [rows][K].  Its adjoint is se_sig_stft of (dy / envelope) followed by the
 * irfft weights, which se_train_ola_bwd and se_train_mask_bwd apply. */
int se_sig_istft(se_sig *g, const float *spec, int rows, float *wav, void *stream);
/* utility.over_add + the K/2 strip (utility.py:373-403, CRN.py:587-588) on segment-major yseg [nseg][B][K] -> out [B][L]; skip = K/2
 * when realtime_process padded the input (flag=False), else 0.  bwd: gseg [nseg][B][K] = adjoint(dout) / envelope. */
int se_train_ola_fwd(se_sig *g, const float *yseg, float *out, int B, int64_t L, int64_t skip, void *stream);
int se_train_ola_bwd(se_sig *g, const float *dout, float *gseg, int B, int nseg, int64_t L, int64_t skip, void *stream);
/* The same three stages for a batch of chunk chains (data_c.py:60-84: every utterance has its own length and its own flag), additions
 * at ABI 4.  off0 / len / skip: DEVICE int64 [B].  se_sig_stft_rows: wav [B][M][Lmax]; utterance b is wav[b][m][i] for 0 <= i < len[b] and
 * ZERO elsewhere (enforced here, whatever the caller padded with); its segment y starts at off0[b] + y * seg_off; spec as se_sig_stft.
 * se_train_ola_fwd_rows: out [B][Lmax], out[b][len[b]:] = 0; _bwd_rows never reads dout[b][len[b]:].  Row b equals the scalar call on
 * that utterance alone bit for bit.  nseg must cover the longest utterance (train_stages.ragged_geometry). */
int se_sig_stft_rows(se_sig *g, const float *wav, int B, int M, int64_t Lmax, const int64_t *off0, const int64_t *len, int64_t seg_off, int nseg, float *spec,
                     void *stream);
int se_train_ola_fwd_rows(se_sig *g, const float *yseg, float *out, int B, int64_t Lmax, const int64_t *skip, const int64_t *len, void *stream);
int se_train_ola_bwd_rows(se_sig *g, const float *dout, float *gseg, int B, int nseg, int64_t Lmax, const int64_t *skip, const int64_t *len, void *stream);
/* per-stream slab gather: dst[b][x] = src[idx[b] * sN + b * sB + x] for x < X, zeros where idx[b] < 0 (idx: device int64 [B]).  src
 * [N + 1][B][X] (sN = B * X, sB = X): every utterance's carried state at its own last segment; src [1][B][X] with idx 0 / -1: the first
 * slab of a mixed-flag batch (the carried row, or zeros after a reset). */
int se_train_slab_gather(const float *src, const int64_t *idx, float *dst, int B, int64_t X, int64_t sN, int64_t sB, void *stream);
/* features (CRN.py:463-467): spec [S][M][T][F][2] -> feat [S][2M-1][T][F] (no backward: the input carries no gradient) */
int se_train_feat(const float *spec, float *feat, int S, int M, int T, int F, int atan2_phase, void *stream);
/* decompress_cIRM + complex multiply with microphone 0 (utility.py:439-442, CRN.py:491-495): x [S][2][T][F] -> Y [S][T][F][2];
 * bwd takes dY = se_sig_stft(gseg) (raw) and returns dx */
int se_train_mask_fwd(const float *x, const float *spec, float *Y, int S, int M, int T, int F, void *stream);
int se_train_mask_bwd(const float *dY, const float *x, const float *spec, float *dx, int S, int M, int T, int F, int n_fft, void *stream);
/* y = GlobalLayerNorm(act(x)) (CRN.py:135-149) per stream; element (s, c, t, f) of x at s*xS + c*xC + t*xT + f (same form for y, dy);
 * mode 0: affine per channel, mode 1: per feature c*Fi + f (last=True); act 0 none / 1 ReLU / 2 ELU; Fo >= Fi zero-fills the
 * decoder's frequency pad (CRN.py:389-392); stats [S][2] = mean, 1/(sqrt(var+eps)+eps).
 * bwd: dx (x strides) = gradient w.r.t. the PRE-activation x; dw_part / db_part / dpre_part [S][NA] slabs (NA = C or C*Fi; any may be
 * NULL), dpre = per-channel sum of dx = the producing convolution's bias gradient. */
int se_train_gln_fwd(const float *x, int64_t xS, int64_t xC, int64_t xT, float *y, int64_t yS, int64_t yC, int64_t yT, const float *w, const float *b,
                     float *stats, int S, int C, int T, int Fi, int Fo, int mode, int act, int eps_mode, void *stream);
int se_train_gln_bwd(const float *dy, int64_t dS, int64_t dC, int64_t dT, const float *x, int64_t xS, int64_t xC, int64_t xT, float *dx, const float *w,
                     const float *stats, float *dw_part, float *db_part, float *dpre_part, int S, int C, int T, int Fi, int mode, int act,
                     int eps_mode, void *stream);
/* out_k[j] (+)= sum over the R rows of part_k[r][j], k < 3 (fixed order); _tall: R up to millions via 64-row chunks in ws[ceil(R/64)][n] */
int se_train_colsum(const float *p0, float *o0, int n0, const float *p1, float *o1, int n1, const float *p2, float *o2, int n2, int R, int accumulate,
                    void *stream);
int se_train_colsum_tall(const float *x, int64_t R, int n, float *ws, float *out, int accumulate, void *stream);
/* decoder skip gate (CRN.py:387-396): uv [S][2Co][T][F] = the stacked 1x1 convolutions (residual | residualmask) of the skip tensor,
 * z [S][Co][T][F] = padded gLN(act(deconv)); out = m * act(u) + (1 - m) * z, m = sigmoid(gLN(v)) */
int se_train_skip_fwd(const float *uv, const float *z, const float *nw, const float *nb, float *out, float *stats, int S, int Co, int T, int F, int act,
                      int eps_mode, void *stream);
int se_train_skip_bwd(const float *dout, const float *uv, const float *z, const float *nw, const float *nb, const float *stats, float *duv, float *dz,
                      float *dnw_part, float *dnb_part, float *dbias_part, int S, int Co, int T, int F, int act, int eps_mode, void *stream);
int se_train_add(float *dst, const float *src, int64_t n, void *stream);
int se_train_add3(float *dst, const float *a, const float *b, int64_t n, void *stream);   /* dst = a + b */
/* CRN_ELU deltas (CRN_ELU.py:194-252, 335-340): gated 1x1 pair + norm: tg [S][2C][T][F] = (conv_trans | conv_gated)(a);
 * y = gLN(t * sigmoid(g)); bwd -> dtg and slabs dw_part / db_part [S][C], dbias_part [S][2C].  se_train_elu_bwd: in place
 * da -> dy through a = ELU(y) from the saved activation, + the [S][C] slab of per-channel sums.  se_train_pre5: the 5-channel 5x5
 * frequency-dilated pre-conv blocks (C <= 8, vector ALU): mode 0 forward (act 2 stores ELU), 1 input gradient, 2 weight-gradient
 * slab [S][C*C*25]. */
int se_train_gate_fwd(const float *tg, const float *w, const float *b, float *y, int64_t yS, int64_t yC, int64_t yT, float *stats, int S, int C, int T, int F,
                      int eps_mode, void *stream);
int se_train_gate_bwd(const float *dy, int64_t dS, int64_t dC, int64_t dT, const float *tg, const float *w, const float *stats, float *dtg, float *dw_part,
                      float *db_part, float *dbias_part, int S, int C, int T, int F, int eps_mode, void *stream);
int se_train_elu_bwd(float *da, const float *act, float *dpre_part, int S, int C, int T, int F, void *stream);
int se_train_pre5(int mode, const float *x, const float *xprev, const float *w, const float *bias, const float *dy, float *out, int S, int C, int T, int F,
                  int fd, int act, void *stream);
/* h_{s-1} rows for the recurrent weight gradient (row addressing as se_train_gru_pseq_*) */
int se_train_gru_hprev(const float *out, const float *h0, float *hp, int B, int T, int H, int Tseg, int64_t ldN, int64_t ldB, void *stream);
/* Convolutions with the weights in their checkpoint layout (element (row, col, kf, kt) at w[row*sCo + col*sCi + kf*3 + kt]).
 * kind 0: TemporalConv2d (CRN.py:314: 5x3, stride (2,1), padding (2,0), dilation (1,d), causal with the history rows `xprev`);
 * kind 1 / 2: even / odd output-frequency parity of TemporalConvTranspose2d (CRN.py:369, keeping the last T columns); kind 3: 1x1.
 * The input gradient of kind 0 is kinds 1 + 2 applied to dy with the SAME weight tensor (and vice versa): same index algebra.
 * ws: se_train_conv_ws_floats() floats of scratch for the arrangement the kernel stages (made on the device). */
int se_train_conv_ws_floats(int kind, int Ci, int Co, int T, int Fi, int Fy, int dil);
int se_train_conv_w(int kind, const float *x, const float *xprev, const float *w, int64_t sCo, int64_t sCi, const float *bias, float *y, float *ws,
                    int B, int Ci, int Co, int T, int Fi, int Fy, int dil, int act, int Cy, int cy0, void *stream);
                    /* Cy > 0: y has Cy channels per stream and this launch writes channels [cy0, cy0 + Co) */
/* weight gradients as partial tiles per row split in ws[<= 64][...] (fold with se_train_colsum: fixed order, no atomics).
 * _conv_wgrad_det: C[a][b][ntap] = sum_{batch,t,m} G[a][t][m] * S[b][t-(2-kt)d][2m+kf-2], ntap = 15 (5x3: kind 0 with G = dy, S = x, Sprev =
 * history; the transposed convolution with G = x, S = dy, Sprev = NULL) or 1 (1x1).  _gemm_tn_det: C[Na][Nb] = sum_r A[r][i] B[r][j], both
 * operands row-major [R][.]: dense-layer weight gradients over R rows. */
int se_train_conv_wgrad_det(const float *G, const float *S, const float *Sprev, float *ws, int *nsplit_out, int B, int Ca, int Cb, int T, int Fm,
                            int Fs, int dil, int ntap, void *stream);
int se_train_gemm_tn_det(const float *A, const float *B, float *ws, int *nsplit_out, int64_t R, int Na, int Nb, void *stream);

/* ---- distillation training (reference distillation_crn.py:504-572; csrc/se_distill.hip; ABI-4 additions) ---------------------
 * se_train_add_csum: dst[S][C][X] += src, then part[S][C] = per-(row, channel) sums of the result (fold with se_train_colsum):
 * injects a feature-map gradient into a pre-activation gradient and gives the bias gradient slab.
 * se_distill_*: the feature loss  sum_i mean((v_i - t'_i)^2 * mask_i) / nmaps  with v = BatchNorm2d(W s) (1x1 connector, no
 * bias), t' = max(t, margin_c), margin_c = sum(t[t<0]) / (count(t<0) + 1e-8) per channel, mask = 1 - (v <= t' & t' <= 0).
 * Every map is [S][C][X] (X contiguous per row and channel; teacher and student in the same layout).  training != 0: batch
 * statistics, running_mean / running_var (momentum 0.1, unbiased variance) and num_batches_tracked are updated on the device;
 * training == 0: the running statistics normalise (nn.BatchNorm2d eval).  Cs <= 64, Ct <= 128, nmaps <= 8.
 * fwd writes loss[0] = the total and loss[1 + i] = the mean of map i; ws (se_distill_ws_bytes) carries the statistics to bwd, which
 * takes the upstream gradient gout[0] from device memory and writes ds, dw, dgamma, dbeta (ds may be null: no input gradient).
 * No float atomics: results are bit-reproducible. */
typedef struct {
    const float *s, *t, *w, *gamma, *beta;      /* student [S][Cs][X], teacher [S][Ct][X], W [Ct][Cs], BN affine [Ct] */
    float *running_mean, *running_var;          /* [Ct] */
    int64_t *num_batches_tracked;               /* [1] */
    float *ds, *dw, *dgamma, *dbeta;            /* gradients: [S][Cs][X], [Ct][Cs], [Ct], [Ct] */
    int Cs, Ct, X, pad_;
} se_distill_map;
int se_train_add_csum(float *dst, const float *src, float *part, int S, int C, int64_t X, void *stream);
int64_t se_distill_ws_bytes(const se_distill_map *maps, int nmaps, int S);
int se_distill_fwd(const se_distill_map *maps, int nmaps, int S, int training, void *ws, float *loss, void *stream);
int se_distill_bwd(const se_distill_map *maps, int nmaps, int S, int training, void *ws, const float *gout, void *stream);

/* ---- GeneralBeamformer inference head (reference GeneralBeamformer.py:336-373; csrc/se_gbf.hip; ABI-4 additions) -------------
 * Segment-major streams S = N x B as the se_train_* calls; M = 3 microphones (the head's linear layers are 9 -> H -> 6).
 * S = Nc x B must hold whole segments: the GRU rows are STREAM-major [B][F][Nc][T] (one [B F][Nc T] sequence set per call, the ldN = 0
 * addressing of se_train_gru_pseq_fwd, which any number of streams accepts).
 * se_gbf_psd_fwd: xl [S][4M*9][T][F] (last decoder output, channel ((s*2 + ri)*M + m)*9 + k), spec [S][M][T][F][2] -> the GRU input
 *   rows of both sequence models [B][F][Nc][T][16]: gLN(Phi) over F*T*9 per stream with affine [F*T] (ln_S / ln_N), columns 9..15 zero.
 * se_gbf_seq_fwd: last-layer GRU outputs hS / hN (rows [B][F][Nc][T] of H) -> phi [S][F][T][9] = SequenceModel_S * SequenceModel_N (fc H -> 9,
 *   ReLU, gLN over T x 9 per sequence); yS / yN (may be NULL) receive the two factors.
 * se_gbf_bf_fwd: phi -> Y [S][T][F][2] = sum_m w_m X_m with w = linear.3(gLN_F(ReLU(linear.0(phi)))); wout [S][F][T][6] may be NULL.
 * No atomics; reductions in a fixed order independent of S. */
int se_gbf_psd_fwd(const float *xl, const float *spec, const float *wS, const float *bS, const float *wN, const float *bN, float *rowsS, float *rowsN,
                   int S, int B, int M, int T, int F, void *stream);
int se_gbf_seq_fwd(const float *hS, const float *hN, const float *fcS_w, const float *fcS_b, const float *nS_w, const float *nS_b, const float *fcN_w,
                   const float *fcN_b, const float *nN_w, const float *nN_b, float *phi, float *yS, float *yN, int S, int B, int F, int T, int H, void *stream);
int se_gbf_bf_fwd(const float *phi, const float *spec, const float *w0, const float *b0, const float *g, const float *beta, const float *w3,
                  const float *b3, float *Y, float *wout, int S, int M, int T, int F, int H, void *stream);
/* Backward of the three head stages (training).  Forward statistics are recomputed from the same inputs.  Parameter gradients come out
 * as slabs / planes to fold in a fixed order (se_train_colsum_tall, se_train_gemm_tn_det); no atomics.
 * se_gbf_bf_bwd: dY [S][T][F][2] = raw se_sig_stft of the segment gradient (the irfft weights c_f / n_fft are applied here) ->
 *   dphi [S][F][T][9]; planes over rows r = s*F*T + f*T + t: dpre [r][H] (linear.0 output gradient: linear.0.weight = dpre^T phi,
 *   linear.0.bias = column sums), act [r][H] (linear.3 input), dw [r][8] (beamforming weight gradient, columns 6, 7 zero:
 *   linear.3.weight = dw^T act); pg / pb [S][T][F]: sums over H for linear.2.weight / bias (column sums over S*T rows).
 * se_gbf_seq_bwd: dphi -> dhS / dhN (last-layer GRU output gradients, rows [B][F][Nc][T] of H), dvS / dvN [rows][16] (fc_output_layer
 *   output gradient, columns 9..15 zero: fc weight = dv^T h), part [S*F][54]: per model q at q*27 norm.weight (9), norm.bias (9),
 *   fc_output_layer.bias (9).
 * se_gbf_psd_bwd: drowsS / drowsN (gradients of the GRU input rows [B][F][Nc][T][16], columns 0..8 read) -> dxl [S][4M*9][T][F];
 *   part [S][4][F*T]: ln_S weight, ln_S bias, ln_N weight, ln_N bias.  The noisy spectrum carries no gradient. */
int se_gbf_psd_bwd(const float *xl, const float *spec, const float *wS, const float *bS, const float *wN, const float *bN, const float *drowsS,
                   const float *drowsN, float *dxl, float *part, int S, int B, int M, int T, int F, void *stream);
int se_gbf_seq_bwd(const float *dphi, const float *hS, const float *hN, const float *fcS_w, const float *fcS_b, const float *nS_w,
                   const float *nS_b, const float *fcN_w, const float *fcN_b, const float *nN_w, const float *nN_b, float *dhS, float *dhN,
                   float *dvS, float *dvN, float *part, int S, int B, int F, int T, int H, void *stream);
int se_gbf_bf_bwd(const float *dY, const float *phi, const float *spec, const float *w0, const float *b0, const float *g, const float *beta,
                  const float *w3, float *dphi, float *dpre, float *act, float *dw, float *pg, float *pb, int S, int M, int T, int F, int H,
                  int n_fft, void *stream);

/* ---- GTSA inference (reference GTSA.py:139-307; csrc/se_gtsa.hip; additions at ABI 5) ------------------------------------------------
 * Window-major streams S = Nc x B (s = n B + b).  ONE activation layout x [S][5][T][Fs]: 5 = 2M - 1 features of M = 3 microphones, Fs >= F
 * the row stride (F padded to the GEMM's K % 8; every kernel that writes x writes zeros into the pad).  Even transformer layers take rows
 * (s, c, t) of F; odd layers rows (s, f, t) of 5 at stride T Fs.  T <= 32 frames per window; se_gtsa_limits reports the limits.
 * The rolling key / value buffer of a layer is a tape per (sequence, head): rows [0, maxlen) the carried part
 * kc / vc [(b U + u) Hh + h][maxlen][D], then row maxlen + n T + t = row ((n B + b) U + u) T + t of kn / vn (stride ldk, head h at
 * column h D).  U sequences per utterance (5 on even layers, F on odd), Hh heads of D (3 x 67 / 1 x 5).
 * se_gtsa_feat: spec [S][M][T][F][2] -> x: sqrt(re^2 + im^2 + 1e-10) of every microphone, atan2 phase differences angle_0 - angle_m;
 *   a bin that is exactly zero has phase 0 whatever the signs of its zeros.
 * se_gtsa_attn: out[row ((s U + u) T + t), stride ldo, column h D ..] = softmax_j(|q . k_j G[i][j] / sqrt(model_dim)|) v_j over the
 *   maxlen tape rows [(n + 1) T, (n + 1) T + maxlen) of window n, i = maxlen - T + t, G = exp(-(i - j)^2 / (delta^2 + 1e-8));
 *   q rows like out at stride ldq.  T <= maxlen <= 4096.  Scores and probabilities stay on chip.
 * se_gtsa_tape: ko / vo (same layout as kc / vc, other memory) = the last maxlen tape rows after Nc windows.
 * se_gtsa_addnorm: y = gLN(a + x) for nseq sequences of T rows (a at stride lda, x / y at stride Fs; y may be x): statistics over
 *   T x F, (v - mean) / (sqrt(var + 1e-10) + 1e-8) * w[f] + b[f]; T F <= 8192.
 * se_gtsa_qkv5: the 5 x 5 q / k / v projections of an odd layer -> qkv [S][F][T][16] (q 0..4, k 5..9, v 10..14, 15 zero).
 * se_gtsa_tail5: an odd layer after attention, in place if y = x: att rows [S][F][T] (stride lda) -> linear (5 x 5) + x, gLN (naw, nab),
 *   linear_in [fn][5] + ReLU + linear_out [5][fn] + residual, gLN (niw, nib).  The hidden activation is never stored.
 * se_gtsa_gather3: A [S T][3 * 5][Fs] = frames t - 2, t - 1, t of x; frames before window 0 come from buf [B][5][2][Fs].
 * se_gtsa_out: g rows [S T] (stride ldg: conv_trans at column o, conv_gated at 2F + o) -> gLN over 2F x T of trans * sigmoid(gated)
 *   with affine [2F], decompress_cIRM, times microphone 0 of spec -> Y [S][T][F][2]; tap (may be NULL) [S][2F][T] the mask before
 *   decompress_cIRM.
 * Chunk chains (stream b has cnt[b] <= Nc windows of its own in the pass; cnt a device int64 [B], values outside [0, Nc] clamped):
 * se_gtsa_tape_rows: se_gtsa_tape with every stream's tape ending after its own windows: ko / vo of stream b = tape rows
 *   [cnt[b] T, cnt[b] T + maxlen) - the carried part itself where cnt[b] = 0; cnt[b] = Nc for all b is se_gtsa_tape bit for bit.
 * se_gtsa_lastframes_rows: buf_out [B][5][2][Fs] = frames T - 2, T - 1 of x [(cnt[b] - 1) B + b], buf_in[b] where cnt[b] = 0 (T >= 2).
 * No atomics; reductions in a fixed order independent of S. */
int se_gtsa_limits(int *max_frames, int *max_maxlen, int *max_norm_values);
int se_gtsa_feat(const float *spec, float *x, int S, int M, int T, int F, int Fs, void *stream);
int se_gtsa_attn(const float *q, const float *kn, const float *vn, const float *kc, const float *vc, float *out, const float *delta, int ldq,
                 int ldk, int ldo, int S, int B, int U, int Hh, int D, int T, int maxlen, int model_dim, void *stream);
int se_gtsa_tape(const float *kn, const float *vn, const float *kc, const float *vc, float *ko, float *vo, int ldk, int Nc, int B, int U, int Hh,
                 int D, int T, int maxlen, void *stream);
int se_gtsa_tape_rows(const float *kn, const float *vn, const float *kc, const float *vc, float *ko, float *vo, const int64_t *cnt, int ldk, int Nc,
                      int B, int U, int Hh, int D, int T, int maxlen, void *stream);
int se_gtsa_lastframes_rows(const float *x, const float *buf_in, float *buf_out, const int64_t *cnt, int Nc, int B, int T, int Fs, void *stream);
int se_gtsa_addnorm(const float *a, int lda, const float *x, float *y, const float *w, const float *b, int nseq, int T, int F, int Fs, void *stream);
int se_gtsa_qkv5(const float *x, const float *wq, const float *bq, const float *wk, const float *bk, const float *wv, const float *bv, float *qkv,
                 int S, int T, int F, int Fs, void *stream);
int se_gtsa_tail5(const float *att, int lda, const float *x, float *y, const float *wo, const float *bo, const float *naw, const float *nab,
                  const float *win, const float *bin, const float *wout, const float *bout, const float *niw, const float *nib, int S, int T, int F,
                  int Fs, int fn, void *stream);
int se_gtsa_gather3(const float *x, const float *buf, float *A, int S, int B, int T, int Fs, void *stream);
int se_gtsa_out(const float *g, int ldg, const float *nw, const float *nb, const float *spec, float *Y, float *tap, int S, int M, int T, int F,
                void *stream);

/* ---- HiFi-GAN generator inference (csrc/se_hifi.hip; reference Hifi-GAN/hifigan.py:444-656) ------------------------------
 * What the generator needs beyond se_train_conv_w / se_train_gemm and the se_sig_* chain.  Device pointers, fp32, no float atomics,
 * fixed-order reductions; activations [S][C][T][F], S = Nc windows x B utterances, window-major (s = n B + b).  0 or a negative
 * se_status, se_train_last_error() = message.
 * se_hifi_postnet: x [S][2][T][F] -> y [S][2][T][F] through the twelve 1x1 layers, self-gate tanh(v) sigmoid(v) after each; one
 *   workgroup keeps 128 bins of one stream on chip through all layers (f32-input MFMA for the ten 128 x 128 layers).  pack: layer by
 *   layer the weight-norm-folded weight [Co][Ci] then the bias: [128][2], [128], 10 x ([128][128], [128]), [2][128], [2].
 * se_hifi_gate: y[i] = tanh(x[i]) sigmoid(x[i]), n values.
 * se_hifi_skip: out [S][Co][T][Fr] = sigmoid(v) tanh(u) + (1 - sigmoid(v)) z; z = self-gate of yd [S][Co][T][Fy], zero for f >= Fy
 *   (Fy <= Fr); uv [S][2 Co][T][Fr] = u (residual) in channels [0, Co), v (residualmask) in [Co, 2 Co).
 * se_hifi_rows: x [S][C][T][F] -> rows [B][Nc T][C F], row (b, n T + t), column c F + f.
 * se_hifi_lstm: one LSTM layer over TT steps, one launch per step and no waiting between workgroups: gi [B][TT][4H] = x W_ih^T + b_ih
 *   + b_hh (gate order i, f, g, o), h0 / c0 [B][H], whh [4H][H] -> out [B][TT][H], hT / cT [B][H] (other memory than h0 / c0); H % 8 == 0, H <= 1024.
 * se_hifi_seqnorm: o [B][Nc][T][D = C F] (the fc output before its tanh) -> y [S][C][T][F] = (tanh(o) - g) w[d] + bias[d], g the
 *   running mean of the utterance after the window: g = alpha g + (1 - alpha) mean_{T x D}(tanh(o)), alpha = step / (step + D),
 *   step += D per window, starting from mean_in [B] and `step` (zeros and 0: nothing carried); wm [B Nc] scratch (receives g per
 *   window), mean_out [B] = g after the last window.
 * Chunk chains (every row / utterance on its own schedule; a row's arithmetic is bit for bit the plain entry point's on that row alone):
 * se_hifi_lstm_rows: steps = device int32 [B], values in [0, TT], any order: row b runs steps[b] steps; out[b][steps[b]:] = 0,
 *   hT[b] / cT[b] after its own last step (h0[b] / c0[b] at 0 steps); still one launch per step, TT of them, and a workgroup whose
 *   eight rows have all finished returns at once.
 * se_hifi_seqnorm_rows: step, cnt = device int64 [B]: utterance b scans its first cnt[b] of the Nc windows from its own step[b];
 *   mean_out[b] after its own last window (mean_in[b] at cnt[b] = 0); the windows past cnt[b] are normalised by that mean (finite,
 *   nobody's result). */
int se_hifi_postnet(const float *x, const float *pack, float *y, int S, int T, int F, void *stream);
int se_hifi_gate(const float *x, float *y, int64_t n, void *stream);
int se_hifi_skip(const float *yd, const float *uv, float *out, int S, int Co, int T, int Fy, int Fr, void *stream);
int se_hifi_rows(const float *x, float *rows, int Nc, int B, int C, int T, int F, void *stream);
int se_hifi_lstm(const float *gi, const float *h0, const float *c0, const float *whh, float *out, float *hT, float *cT, int B, int TT, int H,
                 void *stream);
int se_hifi_seqnorm(const float *o, const float *w, const float *bias, const float *mean_in, double step, float *wm, float *mean_out, float *y,
                    int Nc, int B, int C, int T, int F, void *stream);
int se_hifi_lstm_rows(const float *gi, const float *h0, const float *c0, const float *whh, float *out, float *hT, float *cT, const int *steps, int B,
                      int TT, int H, void *stream);
int se_hifi_seqnorm_rows(const float *o, const float *w, const float *bias, const float *mean_in, const int64_t *step, const int64_t *cnt, float *wm,
                         float *mean_out, float *y, int Nc, int B, int C, int T, int F, void *stream);
/* HiFi-GAN generator training (csrc/se_hifi.hip, csrc/se_hifi_train.hip; hifigan_training.py): no float atomics.
 * se_hifi_lstm_train_fwd: se_hifi_lstm (the same arithmetic: out, hT, cT bit-equal) that also stores, per step, the activated gates
 *   [B][TT][4H] (i, f, g, o) and the cell cs [B][TT][H].
 * se_hifi_lstm_bwd: the backward sweep of one layer over the R = B Nc (utterance, window) rows of a pass, T steps, one launch per step
 *   from T - 1 down: (h, c) are detached at every window seam, so a row starts from dh_rec = dc = 0.  dout / gates / cs as the forward
 *   left them (row r T + t of [R T][.] is step t of row r = b Nc + n), cprev [R T][H] = c_{t-1} of every row (cs shifted by one step
 *   with the pass's entry cell in front of every utterance: se_train_gru_hprev of cs), whht = W_hh^T [H][4H];
 *   -> dgates [R T][4H], the gradient of gi (and of the recurrent pre-activation); dc [R][H] scratch.
 * se_hifi_seqnorm_bwd: dy [S][C][T][F] -> dout [B][Nc T][D], the gradient of the fc output o before its tanh, through
 *   y = (tanh(o) - g_n) w + b with g_{n-1} detached: e = dy w, d tanh = e - (1 - alpha_n) mean_{T x D}(e), alpha_n = step_n /
 *   (step_n + D), step_n = step + n D; wm [B Nc] = g per window as se_hifi_seqnorm left it; em [S] scratch; pw / pb [S][D] = the
 *   slabs of dw / db (fold with se_train_colsum).
 * se_hifi_gate_bwd: dx = dy (sech^2(x) sigmoid(x) + tanh(x) sigmoid(x) (1 - sigmoid(x))).
 * se_hifi_skip_bwd: the adjoint of se_hifi_skip: duv [S][2 Co][T][Fr], dyd [S][Co][T][Fy] (through the self-gate of yd; the padded
 *   columns f >= Fy give nothing).  se_hifi_rows_bwd: the adjoint of se_hifi_rows.
 * se_hifi_chansum: part[r] = the sum of the X values of row r (double partial sums, fixed tree): x [S][C][T F] -> the [S][C] slab of a
 *   convolution's bias gradient. */
int se_hifi_lstm_train_fwd(const float *gi, const float *h0, const float *c0, const float *whh, float *out, float *hT, float *cT, float *gates, float *cs, int B,
                           int TT, int H, void *stream);
int se_hifi_lstm_bwd(const float *dout, const float *gates, const float *cs, const float *cprev, const float *whht, float *dgates, float *dc, int B, int Nc, int T,
                     int H, void *stream);
int se_hifi_seqnorm_bwd(const float *dy, const float *o, const float *w, const float *wm, double step, float *em, float *dout, float *pw, float *pb, int Nc, int B,
                        int C, int T, int F, void *stream);
int se_hifi_gate_bwd(const float *dy, const float *x, float *dx, int64_t n, void *stream);
int se_hifi_skip_bwd(const float *dout, const float *yd, const float *uv, float *duv, float *dyd, int S, int Co, int T, int Fy, int Fr, void *stream);
int se_hifi_rows_bwd(const float *drows, float *dx, int Nc, int B, int C, int T, int F, void *stream);
int se_hifi_chansum(const float *x, float *part, int64_t rows, int X, void *stream);
/* HiFi-GAN chunk-chain training (the `_rows` twins of the three entries above that depend on a stream's own schedule; a live row's
 * arithmetic is bit for bit the plain entry point's):
 * se_hifi_lstm_train_fwd_rows: se_hifi_lstm_rows (out, hT, cT bit-equal, steps[b] = 0 included) that also stores the activated gates
 *   and the cell of every live step; a finished row's step stores zeros into gates and cs as well as out, so everything the backward
 *   and the weight-gradient GEMMs read is finite whatever the workspace held.
 * se_hifi_lstm_bwd_rows: live = device int32 [B], utterance b's own windows of the pass, 0 .. Nc.  Row r = b Nc + n is swept only
 *   where n < live[b]; a dead row reads none of dout / gates / cs / cprev and its dgates are exact zeros at every step (a tile of 8
 *   dead rows returns before the dot products); a live row's dgates are those of se_hifi_lstm_bwd on the live rows alone.
 * se_hifi_seqnorm_bwd_rows: step, cnt = device int64 [B], as se_hifi_seqnorm_rows takes them: window n of utterance b is at
 *   step[b] + n D; a window n >= cnt[b] reads neither dy nor o and writes zeros to its dout rows and its pw / pb slabs.  All counts
 *   Nc and one common step: bit-equal to se_hifi_seqnorm_bwd. */
int se_hifi_lstm_train_fwd_rows(const float *gi, const float *h0, const float *c0, const float *whh, float *out, float *hT, float *cT, float *gates, float *cs,
                                const int *steps, int B, int TT, int H, void *stream);
int se_hifi_lstm_bwd_rows(const float *dout, const float *gates, const float *cs, const float *cprev, const float *whht, float *dgates, float *dc, const int *live,
                          int B, int Nc, int T, int H, void *stream);
int se_hifi_seqnorm_bwd_rows(const float *dy, const float *o, const float *w, const float *wm, const int64_t *step, const int64_t *cnt, float *em, float *dout,
                             float *pw, float *pb, int Nc, int B, int C, int T, int F, void *stream);

/* ---- 8f-4: synthetic multi-microphone training data on the GPU (csrc/se_synth.hip) -------------------------------------
 * Replaces the reference's CPU/gpuRIR input pipeline for DP training: multichannel.py:37-103 (Single2Multi.simulate: shoebox
 * image-source RIRs, dry source * RIR), augment.py:29-77 (AddNoise.forward), data_c.py:236-250 (dynamic_mix, MAX_AMP guard).
 * All pointers are DEVICE pointers, all calls enqueue on `stream`; 0 or a negative se_status, se_synth_last_error() = message.
 *   se_synth_rir   rir[R][S][M][Lr]: image-source model of R rooms (room[R][3] sizes in m, beta[R][6] wall reflection
 *                  coefficients x0,x1,y0,y1,z0,z1, src[R][S][3], mic[R][M][3]); images -n/2 .. n/2-1 per axis (nx, ny, nz);
 *                  fractional delays by a Hann-windowed sinc of 8 ms; Lr <= 36864
 *   se_synth_fir   y[R][S][M][L] = x[R][S][L] * rir, truncated to L samples (gpuRIR.simulateTrajectory of a static source)
 *   se_synth_mix   the last source is the noise: mix[R][M][L], noise[R][M][L], absmax[R][M] (scratch) */
const char *se_synth_last_error(void);
int se_synth_rir(const float *room, const float *beta, const float *src, const float *mic, int R, int S, int M, int nx, int ny, int nz,
                 float fs, float c, int Lr, float *rir, void *stream);
/* optional second stage of gpuRIR (PARITY UNPINNED): for samples n >= tdiff[r] * fs the image-source response is replaced by a
 * stochastic tail, rms(last 10 ms before Tdiff) * exp(-6.9078 (n - Td) / (T60 fs)) * unit-variance logistic noise from a
 * counter-based hash of (seed, RIR index, n); tdiff / t60 [R] device arrays in seconds */
int se_synth_rir_tail(float *rir, const float *tdiff, const float *t60, int R, int S, int M, int Lr, float fs, uint32_t seed, void *stream);
int se_synth_fir(const float *x, const float *rir, int R, int S, int M, int64_t L, int Lr, float *y, void *stream);
int se_synth_mix(const float *y, const float *snr_db, int R, int S, int M, int64_t L, float max_amp, float *mix, float *noise, float *absmax,
                 void *stream);

#ifdef __cplusplus
}
#endif
#endif /* SE_ENGINE_H */
