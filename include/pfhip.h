/*
 * pfhip.h — plain-C ABI of the MI355X (gfx950) Paraformer acoustic-model forward path.
 *
 * This is the drop-in boundary beneath the reference's `funasr::Model` plug-in seam
 * (onnxruntime/include/model.h:13-46).  Every entry point names the reference interface it replaces
 * (paths relative to the reference root).  Plain C types only; no exceptions cross this boundary;
 * every function returns a pfhip_status and pfhip_last_error() holds a thread-local message.
 *
 * Threading: like the reference's `Model::Forward`, which all decoder threads call concurrently on
 * one shared handle (websocket/bin/funasr-wss-server.cpp:479-481), every entry point taking a
 * pfhip_model* is re-entrant.  A handle owns ONE weight set per device and one or more execution
 * contexts over it (workspace + streams; pfhip_set_inflight): concurrent pfhip_offline_forward calls
 * run on different contexts — merged into packed launches first when pfhip_set_batching is on — and
 * calls that land on the same context are serialised on its lock.
 */
#ifndef PFHIP_H_
#define PFHIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct pfhip_model pfhip_model;

typedef enum {
  PFHIP_OK = 0,
  PFHIP_ERR_ARG = 1,         /* null / out-of-range argument                                   */
  PFHIP_ERR_HIP = 2,         /* a HIP runtime call failed (message has hipGetErrorString)      */
  PFHIP_ERR_FORMAT = 3,      /* manifest / blob malformed or tensor missing                    */
  PFHIP_ERR_UNSUPPORTED = 4, /* configuration outside what the gfx950 kernels are built for    */
  PFHIP_ERR_CAPACITY = 5     /* caller-provided output buffer too small                        */
} pfhip_status;

/* Thread-local description of the last failure on this thread ("" if none). */
const char* pfhip_last_error(void);

/* ---- model lifetime --------------------------------------------------------------------------
 * Replaces Paraformer::InitAsr(am_model, am_cmvn, am_config, token_file, thread_num)
 * (onnxruntime/src/paraformer.cpp:21-53): loads weights + CMVN + config and builds the fbank tables
 * (knf options of paraformer.cpp:24-31).  Weight container: flat little-endian float32 blob + JSON
 * manifest (see asr-2pass_amd/weights.py).  `device` is the HIP device ordinal (one model replica
 * per GPU; SURVEY.md §8e "replicas only"). */
pfhip_status pfhip_create(const char* weight_blob_path, const char* manifest_json_path, int device,
                          pfhip_model** out);
pfhip_status pfhip_create_from_memory(const void* blob, size_t blob_bytes, const char* manifest_json,
                                      int device, pfhip_model** out);
/* The same with the strings the reference itself passes — its own file contract (onnxruntime/include/com-define.h:52-88):
 *   am_model     <dir>/model.onnx | model_quant.onnx (offline-stream.cpp:74-77, tpass-stream.cpp:62,68) | model.torchscript /
 *                model_blade.torchscript (offline-stream.cpp:79-84: TorchScript archives are not opened, the ONNX file of the same
 *                stem beside it is read) | a container x.pfhip.bin (am_config = its manifest)
 *   second_model NULL, or the online model's decoder.onnx / decoder_quant.onnx (paraformer.cpp:56-121: en_model + de_model)
 *   hw_model     NULL, or model_eb.onnx as handed to InitHwCompiler BEFORE InitAsr (offline-stream.cpp:60-72, paraformer.cpp:243-261)
 *   am_cmvn      am.mvn, read as LoadCmvn does (paraformer.cpp:325-360)
 *   am_config    config.yaml (LoadConfigFromYaml / LoadOnlineConfigFromYaml, paraformer.cpp:178-241)
 * The weights are read by a dependency-free protobuf walk (anonymous transposed MatMul initializers named after their layer,
 * LSTM gate order, dynamic quantisation folded back to float32); nothing in a model file is executed.  The converted container
 * is cached beside the source as <stem>.pfhip.{bin,json} and reused while every source file keeps its size and mtime
 * (PFHIP_MODEL_CACHE=0 switches the cache off; a read-only directory is not an error). */
pfhip_status pfhip_create_from_files(const char* am_model, const char* second_model, const char* hw_model, const char* am_cmvn,
                                     const char* am_config, int device, pfhip_model** out);
/* The file-reading step on its own (no device needed): kind = "asr" | "sensevoice" | "vad" | "punc".  The blob / manifest pointers
 * stay valid until pfhip_container_free.  "asr" (and pfhip_create_from_files) tells the acoustic models apart by their initialisers:
 * ctc.ctc_lo.* present and no decoder.output_layer is SenseVoiceSmall (sensevoice-small.cpp:22-56 reads the same three files; the
 * reference goes by the directory's name, offline-stream.cpp:50-56) and gives a container of config.kind "sensevoice", with
 * encoder_conf.tp_blocks as tp_layers; "sensevoice" is the same reader and PFHIP_ERR_FORMAT for any other model. */
typedef struct pfhip_container pfhip_container;
pfhip_status pfhip_read_model_files(const char* kind, const char* model, const char* second, const char* hotword, const char* cmvn,
                                    const char* config, pfhip_container** out);
const float* pfhip_container_blob(const pfhip_container* c, size_t* bytes);
const char* pfhip_container_manifest(const pfhip_container* c);
int pfhip_container_from_cache(const pfhip_container* c);
void pfhip_container_free(pfhip_container* c);
/* What the wire-format walk sees in ONE .onnx file, as JSON: initializer count and bytes, node count, node inputs nobody
 * produces (0 for a file read correctly), torch-style tensors and the sum of their values.  Inspection only. */
pfhip_status pfhip_onnx_summary(const char* path, char* out, size_t cap);
/* Replaces Paraformer::~Paraformer (paraformer.cpp:267-295). */
void pfhip_destroy(pfhip_model* m);

/* Model facts the host adapter needs (Model::GetAsrSampleRate model.h:40; vocab size = logits width). */
int pfhip_sample_rate(const pfhip_model* m);
int pfhip_vocab_size(const pfhip_model* m);
int pfhip_feat_dim(const pfhip_model* m);   /* lfr_m * n_mels (560) */
int pfhip_d_model(const pfhip_model* m);
/* d_model / attention_heads: 128 (Paraformer-large) or 80 (the small online Paraformer).  The reference never fixes this width — it
 * sizes its caches from encoder_conf.output_size as config.yaml states it (paraformer.cpp:225) — so a host that sizes buffers per
 * head asks here. */
int pfhip_head_dim(const pfhip_model* m);

/* ---- offline forward --------------------------------------------------------------------------
 * Replaces the body of Paraformer::Forward / ParaformerTorch::Forward between `float** din` and the
 * greedy token ids (onnxruntime/src/paraformer.cpp:463-589; batched contract
 * onnxruntime/src/paraformer-torch.cpp:301-475): FbankKaldi (:309-323) -> LfrCmvn (:421-461) ->
 * `m_session_->Run` (:541) -> GreedySearch/FindMax (:386-395, util.cpp:63-74).
 *
 * Caller-owned output buffers (any optional pointer may be NULL):
 *   token_ids [batch*max_tokens]  argmax ids, row-major per utterance (first-max-wins)
 *   token_num [batch]             floor(sum alphas) — the reference's outputTensor[1] (paraformer.cpp:547)
 *   n_fires   [batch]             rows of log-probs the graph produced for the utterance (CIF fires)
 *   n_frames  [batch]             LFR frames T (paraformer.cpp:483)
 *   logp      [batch*max_tokens*vocab]  log-probs (only when a WFST decoder consumes them,
 *                                 paraformer.cpp:563-579); rows >= n_fires are untouched
 * An utterance shorter than one fbank window yields token_num = n_fires = 0 (paraformer.cpp:477-480).
 */
typedef struct {
  int32_t* token_ids;
  int32_t* token_num;
  int32_t* n_fires;
  int32_t* n_frames;
  float* logp;
  int32_t max_tokens;
  /* Timestamp models only (the reference's 4-output graph, paraformer.cpp:545-562 `outputTensor.size() == 4`): the
   * x3-upsampled alphas and CIF integrate trace that TimestampOnnx consumes (pfhip_timestamp_onnx below), one row of
   * max_us floats per utterance, us_len[b] = 3 * n_frames[b] valid.  Any of the three may be NULL; all NULL = skip. */
  float* us_alphas;
  float* us_peaks;
  int32_t* us_len;
  int32_t max_us;
} pfhip_out;

/* Host-buffer form: pcm[i] points at n_samples[i] floats in [-1,1) exactly as Model::Forward gets
 * them from Audio::FetchDynamic (onnxruntime/src/audio.cpp:1052-1108).  Does H2D, the forward, D2H. */
pfhip_status pfhip_offline_forward(pfhip_model* m, const float* const* pcm, const int* n_samples,
                                   int batch, const float* hw_emb, int n_hotwords, pfhip_out* out);

/* Cross-request batching for the host-buffer form: with wait_us > 0, concurrent pfhip_offline_forward callers (the
 * server's decoder threads, funasr-wss-server.cpp:479-481) are merged into packed forwards of up to max_utterances
 * utterances.  ONE queue per handle feeds every execution slot (contexts, replica devices): the caller at its front claims an
 * idle slot and runs the batch it gathered while the next caller already gathers the next one.  A caller that finds nothing in
 * flight runs at once (a lone caller never waits); while every slot is busy the gathering is free; only with an idle slot AND
 * other batches executing does a leader wait — at most wait_us — for company.  Results are identical to separate calls.
 * 0 switches it off (default).  Contextual models are merged where pfhip_set_hotword_merging is on (every caller keeps its own
 * hotword sets in the packed forward); calls with at least max_utterances utterances go straight to the least-loaded slot. */
pfhip_status pfhip_set_batching(pfhip_model* m, int wait_us, int max_utterances);

/* Execution contexts: how many offline forwards of this handle may be in flight per device.  The reference shares ONE
 * Ort::Session among all decoder threads (onnxruntime/src/paraformer.cpp:35-41,541; websocket/bin/funasr-wss-server.cpp:479-481);
 * here the threads share one weight set (blob, repacks, LayerNorm-folded copies, front-end tables) and each forward runs on one
 * of n contexts — a workspace, two streams and the state of its last batch, a few KB until its first forward sizes the
 * workspace.  One launch of a large batch fills the chip, but its bandwidth-bound phases (epilogues, FSMN prologue, launch
 * boundaries, the host round trip for the token counts) leave the matrix cores idle; a second and third batch in flight fill
 * those gaps (+8..12 % audio-s/s at 3).  With pfhip_set_batching the merged batches are dealt to idle contexts from ONE queue.
 * n = 1 (default) is one forward at a time.  PFHIP_INFLIGHT=n in the environment applies it to every handle created.
 * Call at initialisation (it may allocate); contexts of a replica group are created on every device.  The device-pointer form
 * (pfhip_offline_enqueue / _fetch), streams, pfhip_profile_* and pfhip_extract_feats use context 0. */
pfhip_status pfhip_set_inflight(pfhip_model* m, int n);
/* Replaces ParaformerTorch::WarmUp, the dummy forward the reference's GPU flavour runs inside InitAsr
 * (onnxruntime/src/paraformer-torch.cpp:59,477-520): one synthetic batch of `batch` utterances x `n_samples` samples through
 * EVERY execution slot (context x device), so that code objects are loaded and each context's workspace is sized before the
 * first request.  Call after pfhip_set_inflight. */
pfhip_status pfhip_warm_up(pfhip_model* m, int batch, int n_samples);
int pfhip_get_inflight(const pfhip_model* m);
/* One entry per execution slot (context x device) of the handle: packed device forwards run there, caller calls and utterances
 * they served.  utterances / forwards > calls / forwards > 1 is cross-request merging at work.  *n_out = slots (also on
 * PFHIP_ERR_CAPACITY). */
typedef struct {
  int32_t device, context;
  int64_t forwards, calls, utterances;
} pfhip_slot_stats;
pfhip_status pfhip_inflight_stats(pfhip_model* m, pfhip_slot_stats* out, int cap, int* n_out);

/* Device-resident form (what bench.py times): d_pcm is ONE device buffer holding the utterances
 * back to back; sample_off/n_samples are host arrays.  All kernels are enqueued on `stream`
 * (a hipStream_t, NULL = the model's own stream); results stay in the model's device workspace until
 * pfhip_offline_fetch.  One host sync happens inside (the CIF token counts size the decoder launch). */
pfhip_status pfhip_offline_enqueue(pfhip_model* m, const float* d_pcm, const int64_t* sample_off,
                                   const int* n_samples, int batch, void* stream);
pfhip_status pfhip_offline_fetch(pfhip_model* m, pfhip_out* out);
/* pfhip_offline_forward for audio that is already in HBM (d_pcm / sample_off / n_samples as pfhip_offline_enqueue; the buffer
 * must be complete and stay untouched until the call returns): the forward and the D2H of the results on the least-loaded
 * execution slot's own stream, synchronous like the host-buffer form.  What bench.py's `value` times from several threads on
 * ONE handle; d_pcm must live on the device of the handle (groups: device 0's slots only would see it — single-device handles). */
pfhip_status pfhip_offline_forward_resident(pfhip_model* m, const float* d_pcm, const int64_t* sample_off, const int* n_samples,
                                            int batch, pfhip_out* out);

/* ---- audio at other sample rates --------------------------------------------------------------------
 * Replaces Audio::WavResample (onnxruntime/src/audio.cpp:259-284), which Audio::LoadPcmwav / LoadPcmwavOnline (:787-857) run
 * when the caller's rate differs from the model's (dest_sample_rate): Kaldi's LinearResample (onnxruntime/src/resample.cpp) with
 * cutoff 0.99 * 0.5 * min(fs_in, fs_out), 6 zero crossings, a fresh resampler per call and flush = true.  Outputs are bitwise
 * the reference's.  Rates: 1000 <= fs <= 192000 Hz with lcm(fs_in, fs_out) <= INT32_MAX (the reference's int32 tick
 * arithmetic); any other pair is PFHIP_ERR_UNSUPPORTED.  The output rate is always the model's (pfhip_sample_rate).
 *
 * Host only (no device): the number of samples n_in samples at fs_in become at fs_out (LinearResample::GetNumOutputSamples with
 * flush, resample.cpp:220-265), -1 for an unsupported pair.  fs_in == fs_out gives n_in. */
int64_t pfhip_resample_len(int fs_in, int fs_out, int64_t n_in);
/* Host buffers in and out: pcm[b] (n_samples[b] floats at fs_in) -> out[b] (room for cap[b] floats; n_out[b] receives the
 * count, also on PFHIP_ERR_CAPACITY).  H2D, the kernel and D2H on one of the handle's execution slots; re-entrant.
 * fs_in == the model's rate is a plain copy (no kernel), as the reference skips WavResample. */
pfhip_status pfhip_resample(pfhip_model* m, const float* const* pcm, const int* n_samples, int batch, int fs_in, float* const* out,
                            const int* cap, int* n_out);
/* pfhip_offline_forward for audio at sample_rate (the server's `audio_fs`, websocket-server.cpp:361-398): the audio is copied to
 * the device at its own rate and resampled there into the execution slot's PCM workspace, then the forward runs as
 * pfhip_offline_forward_resident does, without a host round trip.  Results are those of pfhip_offline_forward on the output of
 * pfhip_resample.  sample_rate == pfhip_sample_rate(m) is exactly pfhip_offline_forward.  Calls at another rate are not merged
 * with other callers (pfhip_set_batching).  Hotwords (through the bank, below) and the timestamp outputs are as there. */
pfhip_status pfhip_offline_forward_rate(pfhip_model* m, const float* const* pcm, const int* n_samples, int batch, int sample_rate,
                                        const float* hw_emb, int n_hotwords, pfhip_out* out);

/* ---- 16-bit PCM in ----------------------------------------------------------------------------------
 * Replaces the host loops of Audio::LoadPcmwav (onnxruntime/src/audio.cpp:787-819) and Audio::LoadPcmwavOnline (:821-857), which
 * turn the little-endian s16 bytes a client sends into floats, `speech_data[i] = (float)speech_buff[i] / scale` with scale 32768,
 * before Model::Forward sees them.  Every *_s16 entry point takes those samples as they arrive (host-endian int16_t; the
 * supported hosts are little-endian) and means by the sample s the float s / 32768.f.  That division is exact, and so is the
 * x 32768 the front end applies again (paraformer.cpp:312-314): the fbank kernel's s16 form loads (float)s with no multiply, the
 * resampler's converts on load, and every output — feats, log-probs, ids, token_num, us_alphas / us_peaks, N-best, VAD scores —
 * is bit for bit that of the f32 sibling fed s / 32768.f.  Half the bytes cross to the device, and no float copy is made on the host.
 * Arguments other than `pcm` are those of the sibling; sample offsets and counts are in samples.  A device buffer of packed s16
 * (pfhip_offline_enqueue_s16, pfhip_offline_forward_resident_s16) needs 2-byte alignment only: an utterance may start at an odd sample.
 * pfhip_offline_fetch / pfhip_offline_fetch_nbest serve both enqueue forms; a range-guard re-run reads the buffer in the format it was
 * enqueued in.
 * Merged callers (pfhip_set_batching, pfhip_set_hotword_merging): f32 and s16 callers share the queue, and a packed forward holds ONE
 * format — the leader takes the queued callers of its own format and leaves the others, in order, for the next leader — so results
 * stay those of separate calls and nothing is converted on the host.  The two streaming families (pfhip_stream_forward*_s16,
 * pfhip_vad_stream_infer*_s16) convert during the one copy the host makes of every sample anyway (the splice caches and the waveform
 * handed to the end-point detector are floats); their merged rounds (pfhip_set_stream_batching, pfhip_set_vad_stream_batching) mix
 * the two formats freely.  pfhip_vad_stream_infer*_s16 still return waves_out as floats: pfhip_vadseg_feed's decibel track reads it. */
pfhip_status pfhip_offline_forward_s16(pfhip_model* m, const int16_t* const* pcm, const int* n_samples, int batch,
                                       const float* hw_emb, int n_hotwords, pfhip_out* out);
pfhip_status pfhip_offline_forward_hwsets_s16(pfhip_model* m, const int16_t* const* pcm, const int* n_samples, int batch,
                                              const float* const* hw_emb, const int* n_hotwords, int n_sets, const int* set_of_utt,
                                              pfhip_out* out);
/* Audio::LoadPcmwav + WavResample (audio.cpp:787-819, 259-284): s16 at sample_rate, resampled on the device */
pfhip_status pfhip_offline_forward_rate_s16(pfhip_model* m, const int16_t* const* pcm, const int* n_samples, int batch,
                                            int sample_rate, const float* hw_emb, int n_hotwords, pfhip_out* out);
pfhip_status pfhip_offline_enqueue_s16(pfhip_model* m, const int16_t* d_pcm, const int64_t* sample_off, const int* n_samples,
                                       int batch, void* stream);
pfhip_status pfhip_offline_forward_resident_s16(pfhip_model* m, const int16_t* d_pcm, const int64_t* sample_off,
                                                const int* n_samples, int batch, pfhip_out* out);

/* ---- hotwords (contextual model) ---------------------------------------------------------------
 *   pfhip_hotword_embed <-> the `hw_m_session->Run` on model_eb.onnx + the per-hotword row selection inside
 *                           Paraformer::CompileHotwordEmbedding (paraformer.cpp:656-685): ids i32 [H,10] (0-padded, last row
 *                           [1,0,...] appended by the caller, :648-651) + lengths [H] -> f32 [H, d] = LSTM output at step len-1.
 *                           The string -> id part (:601-647: split, seg_dict, vocabulary) is host text handling above this.
 *   pfhip_set_hotwords  <-> the `hw_emb` argument of Model::Forward kept resident for pfhip_offline_enqueue;
 *                           pfhip_offline_forward takes hw_emb [H, d] per call like the reference (paraformer.cpp:515-531).
 * A contextual model without hotwords is an error ("hw_emb is null", :516-520); a plain model ignores them. */
int pfhip_is_contextual(const pfhip_model* m);
/* 1 when the model carries the CifPredictorV3 upsampling head (the reference's 4-output graph, paraformer.cpp:545). */
int pfhip_has_timestamp_head(const pfhip_model* m);
pfhip_status pfhip_hotword_embed(pfhip_model* m, const int32_t* hotword_matrix, const int32_t* lengths, int n_hotwords,
                                 float* out);
pfhip_status pfhip_set_hotwords(pfhip_model* m, const float* hw_emb, int n_hotwords);

/* ---- per-utterance hotword sets, kept projected on the device ---------------------------------------
 * Replaces the one `hw_emb` that Model::Forward hands to the session for the whole batch (paraformer.cpp:515-531) where callers
 * with different lists share a batch: every websocket connection of the reference's server brings its own hotword list
 * (websocket-server.cpp:316-359) to each Forward it makes.  n_sets sets (hw_emb[k]: [n_hotwords[k], d] floats) and, per utterance,
 * the index of the set it attends to in the bias decoder (set_of_utt [batch]).  pfhip_offline_forward(..., hw_emb, n_hotwords, ...)
 * is the one-set case.  A contextual model with no set for an utterance is "hw_emb is null" (:516-520); plain models ignore sets.
 *
 * The bias decoder's projected K/V rows of the sets (bias.dec.kv.*, [H, 2d]) are kept in a per-device bank shared by the
 * execution contexts and found again by content (hash + byte compare): a set seen before costs no upload, no GEMM and no
 * synchronise; missing sets are uploaded and projected on the forward's own stream.  The bank is bounded in bytes
 * (pfhip_set_hotword_bank_bytes; default PFHIP_HOTWORD_BANK_MB = 64 per device), evicts least recently used sets, never one a
 * forward in flight uses; a call with a set that cannot be banked projects its sets into per-call buffers.  Set the bound while
 * no forward is in flight (PFHIP_ERR_ARG otherwise); 0 banks nothing.  The pfhip_set_hotwords set is a bank entry that stays. */
pfhip_status pfhip_offline_forward_hwsets(pfhip_model* m, const float* const* pcm, const int* n_samples, int batch,
                                          const float* const* hw_emb, const int* n_hotwords, int n_sets, const int* set_of_utt,
                                          pfhip_out* out);
pfhip_status pfhip_set_hotword_bank_bytes(pfhip_model* m, int64_t bytes);
/* Contextual callers in the merge queue (pfhip_set_batching): on != 0 lets concurrent pfhip_offline_forward[_hwsets] callers of a
 * contextual model share packed forwards, each utterance attending to its caller's set; a caller without hotwords fails alone.
 * Off (default), every contextual call is a forward of its own, bit-identical to a lone call; merged, results are those of
 * separate calls as far as pfhip_set_batching states it for plain models.  The C++ adapters switch it on
 * (PFHIP_HOTWORD_MERGE=0 keeps it off). */
pfhip_status pfhip_set_hotword_merging(pfhip_model* m, int on);
/* Totals over the devices of the handle.  hits / misses / evictions: sets found resident, uploaded, dropped for room; refused:
 * sets the bank could not take; forwards: contextual forwards, per_call_forwards of them from per-call buffers;
 * sets_in_forwards / forwards = distinct sets per packed forward, max_sets_in_forward its maximum. */
typedef struct {
  int64_t hits, misses, evictions, refused;
  int64_t bytes_in_use, bytes_capacity, sets_resident;
  int64_t forwards, per_call_forwards, sets_in_forwards, max_sets_in_forward;
} pfhip_hwbank_stats;
pfhip_status pfhip_hotword_bank_stats(pfhip_model* m, pfhip_hwbank_stats* out);

/* ---- N-best candidates and token confidence (extension) --------------------------------------------
 * The reference has no counterpart: GreedySearch keeps only the arg-max of each row (paraformer.cpp:386-395), and the only other
 * way to a token's probability is the whole logp matrix.  Here the head also selects, per token row, the k best columns and their
 * log-probabilities (topk.hip): larger logit first, equal logits smaller column first (FindMax's rule, util.cpp:63-74), so
 * ids[.., 0] == token_ids[..], any prefix is the answer for a smaller k, and a value equals the logp entry of its column bit for bit
 * where both are asked for.  exp(logp[.., 0]) is the token's confidence.  Off (no nb / k = 0), the forward is exactly what it was. */
typedef struct {
  int32_t k;        /* 1..8 candidates per token row */
  int32_t* ids;     /* [batch * max_tokens * k], row-major per utterance like token_ids; rows >= n_fires untouched */
  float* logp;      /* same shape: log-probabilities, descending; ids[.., 0] == token_ids[..] */
} pfhip_nbest;
/* pfhip_offline_forward_hwsets plus the candidates (n_sets = 0: a plain model's call; nb == NULL: exactly
 * pfhip_offline_forward_hwsets).  max_tokens is out's.  Same route through the merge queue (pfhip_set_batching): callers with
 * different k share a packed forward that computes the largest, each receives its own first k, and a caller without nb receives
 * what it always did.  After a range-guard re-run the candidates are the re-run's, like token_ids.  PFHIP_ERR_ARG for k outside
 * 1..8, a NULL buffer, or a vocabulary smaller than k. */
pfhip_status pfhip_offline_forward_nbest(pfhip_model* m, const float* const* pcm, const int* n_samples, int batch,
                                         const float* const* hw_emb, const int* n_hotwords, int n_sets, const int* set_of_utt,
                                         pfhip_out* out, const pfhip_nbest* nb);
/* The same from 16-bit PCM (what pfhip_offline_forward_hwsets_s16 is to pfhip_offline_forward_hwsets; see "16-bit PCM in" above):
 * token ids, candidates and values are those of the f32 call fed s / 32768.f bit for bit; callers of both formats share the
 * merge queue as those of the other offline calls do (a packed forward holds one format). */
pfhip_status pfhip_offline_forward_nbest_s16(pfhip_model* m, const int16_t* const* pcm, const int* n_samples, int batch,
                                             const float* const* hw_emb, const int* n_hotwords, int n_sets, const int* set_of_utt,
                                             pfhip_out* out, const pfhip_nbest* nb);
/* Device-pointer form: k candidates for every following pfhip_offline_enqueue of this handle (context 0), 0 = off (default).
 * GreedySearch's arg-max stays what pfhip_offline_fetch returns; the candidates stay in the device workspace beside it. */
pfhip_status pfhip_set_nbest(pfhip_model* m, int k);
/* After pfhip_offline_fetch (whose max_tokens lays out the rows here as well): the candidates of that forward, the first nb->k
 * of the k it computed.  PFHIP_ERR_ARG when the last enqueue computed none (no pfhip_set_nbest) or fewer than nb->k. */
pfhip_status pfhip_offline_fetch_nbest(pfhip_model* m, const pfhip_nbest* nb);

/* ---- fire frames: where the CIF scan completed each token (extension) --------------------------------
 * The reference has no counterpart: its only source of token times is the CifPredictorV3 head of the 4-output graph
 * (paraformer.cpp:545, `outputTensor.size() == 4`); a model without that head returns text only.  Every forward, however, runs the
 * CIF scan (cif.hip), which decides frame by frame where each token's integration completes — the acoustic boundary between two
 * tokens.  With fire frames asked for, a sibling of the scan kernel stores the step of each fire: the same statements in the same
 * order plus one store by one lane per token, so token ids, log-probs, token_num and n_fires are bit for bit those of the forward
 * without.  Resolution is one LFR row (pfhip_lfr_frame_ms: lfr_n x 10 ms = 60 ms) against the head's 20 ms; these are not the head's
 * stamps.  Off (the default), every entry point launches exactly what it launches without this section.
 *
 * pfhip_detail: what a forward may return beside pfhip_out (pfhip_out and pfhip_nbest keep their size).
 *   nbest_k / nbest_ids / nbest_logp   the candidates, as pfhip_nbest's k / ids / logp; nbest_k = 0 with NULL buffers = none
 *   fire_frame [batch * max_tokens]    or NULL.  fire_frame[b*max_tokens + j], j < n_fires[b]: the LFR row (0..n_frames[b]-1) token
 *                                      row j fired in, or n_frames[b] where the offline tail slot fired it (the trailing "</s>" row
 *                                      usually).  Non-decreasing in j.  Rows >= n_fires[b] are untouched. */
typedef struct {
  int32_t nbest_k;
  int32_t* nbest_ids;
  float* nbest_logp;
  int32_t* fire_frame;
} pfhip_detail;
/* pfhip_offline_forward_nbest with a pfhip_detail (det == NULL: exactly pfhip_offline_forward_hwsets) and the rate of the audio:
 * sample_rate = 0 or pfhip_sample_rate(m) is the model's own; any other rate is resampled on the device as pfhip_offline_forward_rate
 * does (and, as there, not merged with other callers).  Candidates and fire frames take every route a forward can take: merged
 * callers (pfhip_set_batching, pfhip_set_hotword_merging) each receive their own utterances' rows, whatever the others asked for;
 * each execution context (pfhip_set_inflight) and replica owns its buffer; after a range-guard re-run they are the re-run's, like
 * token_ids.  Timestamp-head models: leave out's three us_* pointers NULL to skip the head.  PFHIP_ERR_ARG for a bad nbest_k / a
 * nbest buffer missing, PFHIP_ERR_CAPACITY where max_tokens is below the longest token sequence. */
pfhip_status pfhip_offline_forward_detail(pfhip_model* m, const float* const* pcm, const int* n_samples, int batch, int sample_rate,
                                          const float* const* hw_emb, const int* n_hotwords, int n_sets, const int* set_of_utt,
                                          pfhip_out* out, const pfhip_detail* det);
/* The same from 16-bit PCM (see "16-bit PCM in" above): bit for bit the f32 call fed s / 32768.f. */
pfhip_status pfhip_offline_forward_detail_s16(pfhip_model* m, const int16_t* const* pcm, const int* n_samples, int batch, int sample_rate,
                                              const float* const* hw_emb, const int* n_hotwords, int n_sets, const int* set_of_utt,
                                              pfhip_out* out, const pfhip_detail* det);
/* Device-pointer forms: on != 0 makes every following pfhip_offline_enqueue[_s16] (context 0) and pfhip_offline_forward_resident[_s16]
 * (whichever slot runs it) of this handle record fire frames; 0 = off (default). */
pfhip_status pfhip_set_fire_frames(pfhip_model* m, int on);
/* fire_frame [batch * max_tokens], as in pfhip_detail, of the CALLING THREAD's last pfhip_offline_fetch or
 * pfhip_offline_forward_resident[_s16] on this handle, laid out by that call's batch and out->max_tokens (pfhip_offline_fetch comes
 * first, as for pfhip_offline_fetch_nbest).  Those calls copy their fire frames into storage of the calling thread before they give
 * the execution slot up, and this call reads only that copy: threads that share a handle (what the resident form is for) each get
 * their own call's, whatever has run on the slot since, and a fetch made on another thread is not seen here.  PFHIP_ERR_ARG when
 * this thread has fetched no forward of the handle or that forward recorded none (no pfhip_set_fire_frames), PFHIP_ERR_CAPACITY
 * when that call's max_tokens was below its longest token sequence. */
pfhip_status pfhip_offline_fetch_fire_frames(pfhip_model* m, int32_t* fire_frame);
/* Milliseconds of audio one LFR row advances: lfr_n x the 10-ms frame shift (60 for the Paraformers).  0 for a NULL handle. */
int pfhip_lfr_frame_ms(const pfhip_model* m);

/* ---- front end only ----------------------------------------------------------------------------
 * Replaces Paraformer::FbankKaldi + LfrCmvn (paraformer.cpp:309-323, 421-461) on their own:
 * feats_out gets sum(n_frames)*feat_dim floats, utterances back to back; n_frames_out [batch]. */
pfhip_status pfhip_extract_feats(pfhip_model* m, const float* const* pcm, const int* n_samples,
                                 int batch, float* feats_out, size_t feats_cap_floats,
                                 int32_t* n_frames_out);

/* ---- chunk-streaming forward ---------------------------------------------------------------------
 * One pfhip_stream per connection = one `funasr::ParaformerOnline` (onnxruntime/src/paraformer-online.cpp),
 * created from the ONLINE model's container; its caches (fbank splice cache, [5|10|5] overlap window,
 * CIF carry, 16 decoder FSMN caches) live in HBM.  Calls on streams of one model are serialised.
 *   pfhip_stream_create   <-> ParaformerOnline::ParaformerOnline + InitCache   (:12-62, 347-384)
 *   pfhip_stream_forward  <-> ParaformerOnline::Forward(din, len, input_finished) (:525-601), i.e.
 *                             ExtractFeats/OnlineLfrCmvn (:147-238), x*sqrt(d)+GetPosEmb (:549-555, 240-268),
 *                             AddOverlapChunk (:397-413), ForwardChunk = encoder Run + CifSearch + decoder Run
 *                             + OnlineGreedySearch (:415-523, 270-345; paraformer.cpp:362-371)
 *   pfhip_stream_reset    <-> Reset + ResetCache (:386-395)
 * token_ids receives the ids of the tokens this call emitted (the reference returns their text); at most
 * 32000 samples per call (the 2-pass server sends 9600, websocket-server-2pass.cpp:135-148). */
typedef struct pfhip_stream pfhip_stream;
pfhip_status pfhip_stream_create(pfhip_model* m, const int* chunk_size /* [3] or NULL = {5,10,5} */,
                                 pfhip_stream** out);
void pfhip_stream_destroy(pfhip_stream* s);
pfhip_status pfhip_stream_reset(pfhip_stream* s);
pfhip_status pfhip_stream_forward(pfhip_stream* s, const float* pcm, int n_samples, int input_finished,
                                  int32_t* token_ids, int cap, int* n_tokens);
/* From 16-bit PCM as Audio::LoadPcmwavOnline reads it (audio.cpp:821-857); see "16-bit PCM in" above. */
pfhip_status pfhip_stream_forward_s16(pfhip_stream* s, const int16_t* pcm, int n_samples, int input_finished,
                                      int32_t* token_ids, int cap, int* n_tokens);
/* Which branch of ParaformerOnline::Forward the stream's last call took: 0 not a final call (or no feature row), 1 the short
 * final call that flushes the look-back cache (:532-540), 2 a final call whose rows fit one last chunk (:557-559; the only one
 * whose non-empty text the reference ends with a blank, :585-587), 3 first chunk + last chunk (:560-579). */
int pfhip_stream_last_path(const pfhip_stream* s);
/* The same call for n_streams connections of ONE model at once (each stream at most once): every connection runs its own
 * ParaformerOnline::Forward control flow, and the encoder windows that are ready are packed into one forward (a 20-row
 * window costs the full weight stream and ~700 launches whatever its size).  Results are identical to n_streams separate
 * pfhip_stream_forward calls.  token_ids[i] has room for cap[i] ids; n_tokens[i] receives the count.
 * Errors are per connection where they can be: a connection whose cap[i] is too small receives no ids and n_tokens[i] =
 * the count it needed, the call returns PFHIP_ERR_CAPACITY, and every OTHER connection of the batch is served as usual
 * (callers merged by pfhip_set_stream_batching each get their own status).  A failure of the shared forward itself
 * (HIP error, more than 72 CIF fires in one chunk) fails all connections and re-initialises their caches (as
 * pfhip_stream_reset), so no stream is left with a half-advanced chunk. */
pfhip_status pfhip_stream_forward_batch(pfhip_stream* const* streams, int n_streams, const float* const* pcm,
                                        const int* n_samples, const int* input_finished, int32_t* const* token_ids,
                                        const int* cap, int* n_tokens);
pfhip_status pfhip_stream_forward_batch_s16(pfhip_stream* const* streams, int n_streams, const int16_t* const* pcm,
                                            const int* n_samples, const int* input_finished, int32_t* const* token_ids,
                                            const int* cap, int* n_tokens);      /* audio.cpp:821-857 */
/* Cross-connection batching behind the per-connection call: with wait_us > 0, concurrent pfhip_stream_forward callers on
 * different streams of model m (the 2-pass server's one-strand-per-connection threads, websocket-server-2pass.cpp:266-297)
 * are merged into one pfhip_stream_forward_batch of up to max_streams connections; the first caller waits at most wait_us.
 * Results are identical to separate calls.  0 switches it off (default). */
pfhip_status pfhip_set_stream_batching(pfhip_model* m, int wait_us, int max_streams);
/* Inspection of the LAST encoder window of the last call: "chunk" [n,560], "enc" [n,d], "alphas" [n],
 * "emb" [fires,d], "logp" [fires,vocab] (log-probs are only kept after pfhip_stream_set_debug(s,1)).
 * set_debug bit 1 = keep log-probs.  The tensors are read from the model's packed workspace: valid until the next forward. */
pfhip_status pfhip_stream_set_debug(pfhip_stream* s, int on);
pfhip_status pfhip_stream_get_tensor(pfhip_stream* s, const char* name, float* dst, size_t cap_floats,
                                     size_t* n_out);
/* N-best candidates, confidences and fire frames per streamed token (an extension: OnlineGreedySearch, paraformer.cpp:362-371,
 * keeps only the arg-max, and the reference's streaming result carries no time).  Per stream, and through every forward entry
 * point above, batched or merged: the packed forward's head computes the largest k of its streams (topk.hip, as offline) and
 * each stream keeps its own first k; the CIF scan records the step in which each token fired and the host turns it into
 * fire_frame: the index, among the LFR rows this stream's front end has emitted since creation, reset or its last final call
 * (first row = 0; one row = lfr_n * 10 ms), of the row the token fired in.  Rows that a two-window final call (:560-579)
 * feeds again keep their numbers, so within that one call fire_frame can step back.  A token fired by the tail slot of a last
 * chunk gets the window's last row.  With k = 0 and fire frames off (default) every call launches what it always launched.
 * k = 0..8 candidates per token (0 = off), fire_frames != 0: also where each token fired.  Applies to the stream's following calls. */
pfhip_status pfhip_stream_set_detail(pfhip_stream* s, int nbest_k, int fire_frames);
typedef struct {
  int32_t k;            /* <= the stream's k; 0 with ids/logp NULL = fire frames only */
  int32_t* ids;         /* [cap * k] row-major, ids[j*k] == the j-th token id the call returned */
  float* logp;          /* [cap * k] descending; bit for bit the logp entry of its column */
  int32_t* fire_frame;  /* [cap] or NULL */
  int32_t cap;          /* token rows the buffers hold */
} pfhip_stream_detail;
/* The detail of the stream's LAST forward (any entry point, batched or merged); valid until its next forward or reset.
 * n_tokens receives the count (the call's n_tokens, also where its token_ids was too small).  PFHIP_ERR_ARG for a k above
 * what the last call computed or fire frames that were off; PFHIP_ERR_CAPACITY (n_tokens = the count needed) when cap is too
 * small.  A failed shared forward and pfhip_stream_reset leave no detail. */
pfhip_status pfhip_stream_last_detail(pfhip_stream* s, const pfhip_stream_detail* d, int* n_tokens);

/* ---- FSMN-VAD forward ---------------------------------------------------------------------------
 *   pfhip_vad_create_from_memory <-> FsmnVad::InitVad (ReadModel + LoadCmvn + InitCache, fsmn-vad.cpp:12-70, 258-263)
 *   pfhip_vad_forward            <-> FsmnVad::FbankKaldi + LfrCmvn + Forward (fsmn-vad.cpp:137-152, 198-238, 72-135):
 *                                    probs [T, n_classes] row-major (class 0 = silence, e2e-vad.h:103); the four
 *                                    [128 x 19] caches stay in HBM and are advanced only when !is_final (:129-134)
 *   pfhip_vad_reset              <-> FsmnVad::InitCache (:258-263) */
typedef struct pfhip_vad pfhip_vad;
pfhip_status pfhip_vad_create_from_memory(const void* blob, size_t blob_bytes, const char* manifest_json, int device,
                                          pfhip_vad** out);
/* FsmnVad::InitVad(vad_model, vad_cmvn, vad_config, thread_num) with the reference's own strings (fsmn-vad.cpp:10-50:
 * <vad-dir>/model.onnx | model_quant.onnx, am.mvn, config.yaml); see pfhip_create_from_files. */
pfhip_status pfhip_vad_create_from_files(const char* vad_model, const char* vad_cmvn, const char* vad_config, int device, pfhip_vad** out);
void pfhip_vad_destroy(pfhip_vad* v);
pfhip_status pfhip_vad_reset(pfhip_vad* v);
int pfhip_vad_num_classes(const pfhip_vad* v);
pfhip_status pfhip_vad_forward(pfhip_vad* v, const float* pcm, int n_samples, int is_final, float* probs,
                               size_t cap_floats, int* n_frames);

/* Same forward, but only the silence posterior (class 0) of each frame comes back — the one column the end-point
 * detector reads (e2e-vad.h:103,607-609): T floats instead of T x 248. */
pfhip_status pfhip_vad_forward_sil(pfhip_vad* v, const float* pcm, int n_samples, int is_final, float* sil_prob,
                                   size_t cap_floats, int* n_frames);
/* From 16-bit PCM as Audio::LoadPcmwav reads it (audio.cpp:787-819); see "16-bit PCM in" above. */
pfhip_status pfhip_vad_forward_sil_s16(pfhip_vad* v, const int16_t* pcm, int n_samples, int is_final, float* sil_prob,
                                       size_t cap_floats, int* n_frames);

/* ---- the decibel track on the device, files in company -----------------------------------------------------------------------
 * The end-point detector reads, beside the silence posterior, the energy of every 25-ms frame (E2EVadModel::ComputeDecibel,
 * e2e-vad.h:437-452).  pfhip_vad_forward_sil_energy[_s16] is pfhip_vad_forward_sil[_s16] that also returns those energies,
 * computed on the device from the PCM the forward has copied there anyway: energy[f] = sum_{i < 400} x[160 f + i]^2 for the
 * *n_energy = (n_samples < 400 ? 0 : 1 + (n_samples - 400) / 160) frames of THIS call's samples — one fp32 accumulator, i ascending,
 * products rounded to fp32: bit for bit the host loop, for s16 input that of s / 32768.f.  Hand them to pfhip_vadseg_feed_energy,
 * which takes the logarithm on the host (the device's log10 is not glibc's).  sil_prob, *n_frames, is_final and the caches are
 * exactly those of pfhip_vad_forward_sil (same launches, bit-identical scores).  energy may be NULL (count only); cap_energy <
 * *n_energy -> PFHIP_ERR_CAPACITY with *n_energy holding the count. */
pfhip_status pfhip_vad_forward_sil_energy(pfhip_vad* v, const float* pcm, int n_samples, int is_final, float* sil_prob,
                                          size_t cap_floats, int* n_frames, float* energy, size_t cap_energy, int* n_energy);
pfhip_status pfhip_vad_forward_sil_energy_s16(pfhip_vad* v, const int16_t* pcm, int n_samples, int is_final, float* sil_prob,
                                              size_t cap_floats, int* n_frames, float* energy, size_t cap_energy, int* n_energy);
/* n_files COMPLETE files in one pass: every file is scored as an is_final = 1 call on a fresh object — zeroed caches in, nothing
 * carried out (fsmn-vad.cpp:129-134) — so the handle's own carried caches are neither read nor written.  Arrays of the per-file
 * arguments above.  The files' samples go to one device buffer as they are (no host copy, no conversion); one fbank launch, one
 * LFR/CMVN that pads every file at its own edges, one network pass over the packed rows, one energy launch, one synchronise.  A file
 * shorter than one window has n_frames = n_energy = 0.  Errors are per file where they can be: a file whose sil_prob or energy
 * buffer is too small receives its counts and nothing else, the others are served, the call returns PFHIP_ERR_CAPACITY.
 * Numerics: energies are exact (bitwise those of separate calls).  The silence posteriors are those of separate calls up to the
 * GEMM dispatch: the GEMM kernel is picked from the row count, so a file's rows may run on another kernel in company than alone —
 * as one file scored whole and in 1-s slices already may.  Both are within the VAD tolerance against the reference (2e-5). */
pfhip_status pfhip_vad_forward_sil_batch(pfhip_vad* v, const float* const* pcm, const int* n_samples, int n_files, float* const* sil_prob,
                                         const size_t* cap_floats, int* n_frames, float* const* energy, const size_t* cap_energy,
                                         int* n_energy);
pfhip_status pfhip_vad_forward_sil_batch_s16(pfhip_vad* v, const int16_t* const* pcm, const int* n_samples, int n_files,
                                             float* const* sil_prob, const size_t* cap_floats, int* n_frames, float* const* energy,
                                             const size_t* cap_energy, int* n_energy);
/* Merge concurrent pfhip_vad_forward_sil_energy[_s16] callers (one decoder thread per file) into pfhip_vad_forward_sil_batch passes
 * of up to max_files files: only calls with is_final = 1 on a handle that carries no state (no non-final call since create /
 * pfhip_vad_reset) are merged, every other call runs alone as before.  A caller that finds the handle idle runs at once (a lone
 * caller never waits); one that arrives while a pass runs leads the next pass and waits up to wait_us for company.  A pass holds
 * ONE sample format, the leader's; callers of the other format form the next pass.  wait_us = 0 or max_files = 1: off (default).
 * pfhip_vad_batch_stats: packed passes so far (merged or called directly), the files they scored, the most files in one pass. */
pfhip_status pfhip_set_vad_batching(pfhip_vad* v, int wait_us, int max_files);
pfhip_status pfhip_vad_batch_stats(pfhip_vad* v, long long* passes, long long* files, int* max_files);

/* ---- online FSMN-VAD: one pfhip_vad_stream per connection = one `funasr::FsmnVadOnline` --------------------------------
 * (onnxruntime/src/fsmn-vad-online.cpp; built on the offline handle like FsmnVadOnline(FsmnVad*), :206-219).
 *   pfhip_vad_stream_infer <-> FsmnVadOnline::Infer up to the scorer (:135-147): ExtractFeats with input_cache_ /
 *                              lfr_splice_cache_ / reserve_waveforms_ (:11-88), OnlineLfrCmvn (:90-133), Forward with this
 *                              connection's caches.  sil_prob receives the silence posterior of the *n_frames rows this call
 *                              produced; waves_out the waveform FsmnVadOnline hands to vad_scorer for the same rows (:148) —
 *                              feed both to pfhip_vadseg_feed(online = 1).  A final call is scored against zeroed caches and
 *                              resets the object, as the reference does (Reset/ResetCache inside ExtractFeats, :84-87).
 *   pfhip_vad_stream_reset <-> Reset + ResetCache (:160-163, fsmn-vad-online.h:59-63) */
typedef struct pfhip_vad_stream pfhip_vad_stream;
pfhip_status pfhip_vad_stream_create(pfhip_vad* v, pfhip_vad_stream** out);
void pfhip_vad_stream_destroy(pfhip_vad_stream* vs);
pfhip_status pfhip_vad_stream_reset(pfhip_vad_stream* vs);
pfhip_status pfhip_vad_stream_infer(pfhip_vad_stream* vs, const float* pcm, int n_samples, int input_finished, float* sil_prob,
                                    size_t cap_floats, int* n_frames, float* waves_out, size_t waves_cap, int* n_waves);

/* From 16-bit PCM as Audio::LoadPcmwavOnline reads it (audio.cpp:821-857); waves_out stays f32. */
pfhip_status pfhip_vad_stream_infer_s16(pfhip_vad_stream* vs, const int16_t* pcm, int n_samples, int input_finished, float* sil_prob,
                                        size_t cap_floats, int* n_frames, float* waves_out, size_t waves_cap, int* n_waves);

/* The same call for n_streams connections of ONE pfhip_vad at once (arrays of the per-connection arguments above): the 2-pass
 * server's websocket handlers each call FsmnVadOnline::Infer per 600 ms message (websocket-server-2pass.cpp:85-117 ->
 * funasrruntime.cpp:516-532); issued together they share every launch (fbank, OnlineLfrCmvn rows, the 11 GEMMs, the FSMN
 * memory with per-connection caches), so a round of N connections costs about what one call does.  Results are identical to
 * n_streams separate calls.  A stream may appear only once per batch. */
pfhip_status pfhip_vad_stream_infer_batch(pfhip_vad_stream* const* streams, int n_streams, const float* const* pcm,
                                          const int* n_samples, const int* input_finished, float* const* sil_prob,
                                          const size_t* cap_floats, int* n_frames, float* const* waves_out,
                                          const size_t* waves_cap, int* n_waves);

pfhip_status pfhip_vad_stream_infer_batch_s16(pfhip_vad_stream* const* streams, int n_streams, const int16_t* const* pcm,
                                              const int* n_samples, const int* input_finished, float* const* sil_prob,
                                              const size_t* cap_floats, int* n_frames, float* const* waves_out,
                                              const size_t* waves_cap, int* n_waves);      /* audio.cpp:821-857 */

/* Merge concurrent pfhip_vad_stream_infer callers (one thread per connection, as the reference's websocket handlers are) into
 * batched passes: wait_us > 0 and max_streams > 1 make the first caller wait up to wait_us for others.  Default: off. */
pfhip_status pfhip_set_vad_stream_batching(pfhip_vad* v, int wait_us, int max_streams);

/* ---- VAD end-point detector (host logic) -----------------------------------------------------------
 * `funasr::E2EVadModel` (onnxruntime/src/e2e-vad.h:268-783, WindowDetector :181-266, VADXOptions defaults :78-107)
 * restated on the host: sequential threshold / window logic over ~100 frames per second, no device work.
 *   pfhip_vadseg_feed <-> E2EVadModel::operator()(score, waveform, is_final, online, max_end_sil,
 *                         max_single_segment_time, speech_noise_thres, sample_rate) (:303-362); segments are written as
 *                         (start_ms, end_ms) pairs, -1 = "open" in online mode.  *n_segments > cap_pairs -> PFHIP_ERR_CAPACITY. */
typedef struct pfhip_vadseg pfhip_vadseg;
pfhip_status pfhip_vadseg_create(pfhip_vadseg** out);
void pfhip_vadseg_destroy(pfhip_vadseg* s);
pfhip_status pfhip_vadseg_reset(pfhip_vadseg* s);
pfhip_status pfhip_vadseg_feed(pfhip_vadseg* s, const float* sil_prob, int n_frames, const float* waveform,
                               int n_samples, int is_final, int online, int max_end_sil, int max_single_segment_time,
                               float speech_noise_thres, int sample_rate, int32_t* segments, int cap_pairs,
                               int* n_segments);

/* The same call on frame energies instead of samples (pfhip_vad_forward_sil_energy, pfhip_op_frame_energy): energy[n_energy] are
 * the sums of squares of the 25-ms frames of the n_samples new samples; the decibel track is (float)(10 * log10(e + 0.000001)) in
 * double arithmetic, the expression of ComputeDecibel, and the sample accounting runs on n_samples — the segments are exactly those
 * of pfhip_vadseg_feed on the waveform.  n_energy must be the frame count of n_samples at sample_rate (n < 25 ms ? 0 :
 * 1 + (n - 25 ms) / 10 ms): anything else is PFHIP_ERR_ARG.  Online and offline modes. */
pfhip_status pfhip_vadseg_feed_energy(pfhip_vadseg* s, const float* sil_prob, int n_frames, const float* energy, int n_energy,
                                      int n_samples, int is_final, int online, int max_end_sil, int max_single_segment_time,
                                      float speech_noise_thres, int sample_rate, int32_t* segments, int cap_pairs,
                                      int* n_segments);

/* ---- token time stamps (host logic) ------------------------------------------------------------------
 * `funasr::TimestampOnnx` (onnxruntime/src/util.cpp:838-963) restated on the host: us_alphas / us_cif_peak [3T] of the
 * time-stamp model + the number of recognised tokens (without "</s>") -> (begin_s, end_s) spans; spans[3*i+2] != 0 marks
 * an inserted <sil>.  us_alphas is rescaled in place like the reference's by-reference argument. */
pfhip_status pfhip_timestamp_onnx(float* us_alphas, const float* us_cif_peak, int n_frames3, int n_chars, float begin_time_ms,
                                  float total_offset, float* spans, int cap_spans, int* n_spans);
/* `funasr::PostProcess` (onnxruntime/src/util.cpp:720-836), host string handling: n hypothesis tokens (vocabulary strings,
 * UTF-8) + their (begin_s, end_s) stamps -> "<text> | <b0>, <e0>,<b1>, <e1>..." exactly as Paraformer::GreedySearch returns
 * it in time-stamp mode; special tokens dropped, "@@" pieces merged, Latin words spaced.  *n_out = strlen (cap >= +1). */
pfhip_status pfhip_post_process(const char* const* chars, const float* stamps, int n, char* out, int cap, int* n_out);
/* Token spans from fire frames (extension; the reference has no counterpart: TimestampOnnx above, fed by the head of
 * paraformer.cpp:545, is its only source of stamps).  fire_frame [n_fires] as pfhip_detail returns it for one utterance, n_chars
 * <= n_fires the recognised tokens to stamp (without "</s>"), n_frames the utterance's LFR rows, frame_ms = pfhip_lfr_frame_ms.
 * Writes (begin_s, end_s, is_sil) triplets exactly as pfhip_timestamp_onnx does, so pfhip_post_process takes them unchanged.
 * The rule has no constants of its own; it uses TimestampOnnx's two (util.cpp:838-963) as times: MAX_TOKEN_DURATION = 30 x 20 ms =
 * 600 ms and START_END_THRESHOLD = 5 x 20 ms = 100 ms.  In frames, with e[-1] = 0 and maxtok = 600 / frame_ms, for k = 0..n_chars-1:
 *   e[k] = min(fire_frame[k] + 1, n_frames)        the token ends with the row it fired in
 *   b[k] = max(e[k-1], e[k] - maxtok)              and is at most MAX_TOKEN_DURATION long
 *   b[k] > e[k-1]: a <sil> span [e[k-1], b[k]] first; then the token [b[k], e[k]]
 * after the last token: (n_frames - e[last]) * frame_ms > 100 -> a <sil> span [e[last], n_frames], else the last token ends at
 * n_frames.  Seconds = frames * frame_ms / 1000 + begin_time_ms / 1000.  Resolution is one LFR row; two fires in one row give a
 * zero-length token.  No real model has validated the rule against the head's stamps: it is not claimed to equal them.
 * Known answer: n_frames = 40, frame_ms = 60, fire_frame = {4, 9, 30, 33, 40} (the fifth is the tail slot's "</s>"), n_chars = 4 ->
 *   token [0.00, 0.30]  token [0.30, 0.60]  <sil> [0.60, 1.26]  token [1.26, 1.86]  token [1.86, 2.04]  <sil> [2.04, 2.40]
 * PFHIP_ERR_ARG: n_chars > n_fires, a negative argument, frame_ms <= 0, a NULL pointer; PFHIP_ERR_CAPACITY: cap (in triplets) too
 * small, *n_spans = the count needed; n_chars = 0: no spans. */
pfhip_status pfhip_cif_timestamps(const int32_t* fire_frame, int n_fires, int n_chars, int n_frames, float frame_ms,
                                  float begin_time_ms, float* spans, int cap, int* n_spans);

/* ---- CT-Transformer punctuation forward ------------------------------------------------------------
 *   pfhip_punc_create_from_memory <-> CTTransformer::InitPunc session load (ct-transformer.cpp:14-37)
 *   pfhip_punc_infer              <-> CTTransformer::Infer (ct-transformer.cpp:162-204): ids [n] -> punctuation id
 *                                     per token = first maximum over the first CANDIDATE_NUM-1 classes; logits_out
 *                                     (optional) gets the [n, n_classes] scores.  Tokenisation and the 20-token
 *                                     mini-sentence bookkeeping of AddPunc (:39-155) stay on the host above this.
 * Served: d_model % 4 == 0, d_model <= 1024, d_model % n_head == 0, 1 <= d_model / n_head <= 64, ffn % 128 == 0, ffn <= 2048,
 * FSMN kernel 11, sanm_shift 0 or 5, 2 <= n_punc <= 128 (256 / 8 / 1024 x 4, the zh-cn model; 516 / 12 / 2048 x 12, the large
 * cn-en model as recalled); anything else is PFHIP_ERR_UNSUPPORTED with the range and the values in pfhip_last_error. */
typedef struct pfhip_punc pfhip_punc;
pfhip_status pfhip_punc_create_from_memory(const void* blob, size_t blob_bytes, const char* manifest_json, int device,
                                           pfhip_punc** out);
/* CTTransformer::InitPunc(punc_model, punc_config, token_file, thread_num)'s session load with the reference's own strings
 * (ct-transformer.cpp:14-37: <punc-dir>/model.onnx | model_quant.onnx, config.yaml; model_conf.punc_list goes into the manifest's
 * config.punc_list for the host tokenizer); see pfhip_create_from_files. */
pfhip_status pfhip_punc_create_from_files(const char* punc_model, const char* punc_config, int device, pfhip_punc** out);
void pfhip_punc_destroy(pfhip_punc* p);
int pfhip_punc_num_classes(const pfhip_punc* p);
pfhip_status pfhip_punc_infer(pfhip_punc* p, const int32_t* ids, int n, int32_t* punc_out, float* logits_out);
/* Realtime variant <-> CTTransformerOnline::Infer(input_data, nCacheSize) (ct-transformer-online.cpp:154-223): the
 * VadMask of :225-240 (queries before cache_size-1 do not see tokens from cache_size on) is applied in every attention
 * block, because the reference feeds that one mask to both `vad_mask` and `sub_masks` (:182-197).  The model's FSMN
 * look-ahead is the container's `sanm_shift` (0 or 5). */
pfhip_status pfhip_punc_infer_online(pfhip_punc* p, const int32_t* ids, int n, int cache_size, int32_t* punc_out,
                                     float* logits_out);
/* n_seq sequences in one packed device pass (positions, FSMN memory and attention per sequence): results identical to n_seq
 * separate pfhip_punc_infer calls (cache_size == NULL) / pfhip_punc_infer_online calls (cache_size[b] per sequence).
 * pfhip_set_punc_batching(wait_us > 0, max_sequences > 1) merges concurrent single-sequence callers (one AddPunc per handler
 * thread) into such passes; offline and realtime calls are never mixed in one pass.  Default: off. */
pfhip_status pfhip_punc_infer_batch(pfhip_punc* p, const int32_t* const* ids, const int* n, const int* cache_size, int n_seq,
                                    int32_t* const* punc_out);
pfhip_status pfhip_set_punc_batching(pfhip_punc* p, int wait_us, int max_sequences);
/* AddPunc's mini-sentence loop on token ids (ct-transformer.cpp:39-155): 20-token mini-sentences, the tail after the last
 * sentence end carried into the next Infer, forced period at the last comma beyond CACHE_POP_TRIGGER_LIMIT carried tokens,
 * sentence-final fix-up.  punc_out receives one punctuation id per token and, when the text does not end in "。"/"？", one
 * extra PERIOD_INDEX (the reference appends the character): *n_out = n or n + 1 (cap >= n + 1).  The tokeniser and the
 * string assembly stay on the host above this. */
pfhip_status pfhip_punc_add_punc(pfhip_punc* p, const int32_t* ids, int n, int32_t* punc_out, int cap, int* n_out);

/* ---- SenseVoiceSmall, offline (a container with config.kind == "sensevoice") --------------------
 * The reference builds SenseVoiceSmall instead of Paraformer when the model directory's name says so (offline-stream.cpp:50-56) and
 * runs it one utterance at a time (sensevoice-small.cpp:575-690 refuses batch_in != 1); here utterances are packed as everywhere.
 * Model widths and wiring are recalled from upstream FunASR: no SenseVoice file was available when this was written.
 *   pfhip_is_ctc          1 for such a handle.  Every Paraformer forward, pfhip_stream_create and pfhip_set_batching return
 *                         PFHIP_ERR_UNSUPPORTED on it, and pfhip_svs_forward does on a Paraformer handle.
 *   pfhip_svs_set_batching   pfhip_set_batching for such a handle (which keeps refusing it; PFHIP_ERR_UNSUPPORTED here on a
 *                         Paraformer handle and on a multi-device group): concurrent pfhip_svs_forward[_spans][_s16] callers
 *                         are merged into packed forwards by the rules stated at pfhip_set_batching (a lone caller on an idle
 *                         device runs at once, one sample format per packed forward, wait_us = 0: off), each with its own lid /
 *                         textnorm per utterance, its own buffers and its own max_tokens (too small: that caller alone gets
 *                         PFHIP_ERR_CAPACITY).  A caller asking for `logp` costs the others nothing: the fused head runs over all
 *                         rows and the unfused chunks over that caller's rows only.  Results are those of separate calls up to
 *                         the near-tie statement made for merged Paraformer callers (log-probs 1e-4).
 *   pfhip_svs_lid     <-> lid_map (sensevoice-small.h:121-129) with the look-up of sensevoice-small.cpp:597-602: "auto" 0, "zh" 3,
 *                         "en" 4, "yue" 7, "ja" 11, "ko" 12, "nospeech" 13; any other string (or NULL) 0.
 *   pfhip_svs_forward <-> SenseVoiceSmall::Forward (sensevoice-small.cpp:575-690): LfrCmvn features behind the four prompt rows
 *                         embed[lid], embed[1], embed[2], embed[textnorm] (textnorm 14 = with ITN, 15 = without, :603-605), the graph,
 *                         and the frame loop of CTCSearch (:331-347: arg-max per frame, first maximum wins; a frame is kept when
 *                         its id is not the blank and differs from the previous frame's).  The text assembly of :348-375 stays on
 *                         the host above this.  lid / textnorm are per utterance, each in 0..15 (PFHIP_ERR_ARG before any launch).
 *                         An utterance of fewer than 400 samples has no rows at all, prompt rows included, and token_num 0 (the
 *                         reference returns "" without running the graph, :584-587).
 * pfhip_svs_out: ids / token_num as pfhip_out's token_ids / token_num — the kept ids [batch][max_tokens], the four leading tag ids
 * (language, emotion, event, ITN) included; PFHIP_ERR_CAPACITY when max_tokens is below the longest kept sequence.  Optional, NULL to
 * skip: tok_frame / tok_logp [batch][max_tokens] = the 0-based row (prompt rows counted) at which a kept run starts and that frame's
 * log-prob; frame_ids / frame_logp packed [sum rows] with frame_len [batch] = rows per utterance (T + 4, or 0); logp = the full
 * log-softmax rows [sum rows][vocab] for a host search (logp_cap_floats too small: PFHIP_ERR_CAPACITY) — asking for them takes the
 * unfused head (GEMM + log-softmax over chunks of 2048 rows: at most 2 x 2048 x vocab floats of scratch, never rows x vocab). */
int pfhip_is_ctc(const pfhip_model* m);
int pfhip_svs_lid(const char* svs_lang);
pfhip_status pfhip_svs_set_batching(pfhip_model* m, int wait_us, int max_utterances);
typedef struct pfhip_svs_out {
  int32_t* ids; int32_t* token_num; int max_tokens;
  int32_t* tok_frame; float* tok_logp;
  int32_t* frame_ids; float* frame_logp;
  int32_t* frame_len;
  float* logp; size_t logp_cap_floats;
} pfhip_svs_out;
pfhip_status pfhip_svs_forward(pfhip_model* m, const float* const* pcm, const int* n_samples, int batch, const int32_t* lid,
                               const int32_t* textnorm, pfhip_svs_out* out);
pfhip_status pfhip_svs_forward_s16(pfhip_model* m, const int16_t* const* pcm, const int* n_samples, int batch, const int32_t* lid,
                                   const int32_t* textnorm, pfhip_svs_out* out);
/* CTC forced alignment: where each token of a given sequence begins and ends (upstream FunASR's output_timestamp for SenseVoice,
 * recalled; nothing of it is in the reference tree).  tokens[b][0 .. n_tokens[b]) is aligned against the rows that the CALLING
 * THREAD's last pfhip_svs_forward[_s16] on this handle left in its execution context — the lifetime rule of pfhip_get_tensor: valid
 * until that context runs its next forward (a later forward of ANOTHER thread that landed on the same context included: the call then
 * returns PFHIP_ERR_ARG instead of aligning against rows that are not the caller's, and the caller goes without spans or repeats
 * the pair) — so `batch` must equal that forward's.  After a MERGED forward (pfhip_svs_set_batching) the rows are the caller's own
 * sub-range of the packed batch, under the same lifetime rule; never another caller's.  The frames are the speech rows only (the four
 * prompt rows are no CTC rows), so tokens[b] are ids AFTER the four leading tags: ids[b][4:] of the forward for the greedy text, or
 * any other sequence (a search result, a transcript the caller has).  The blank is the container's blank_id.  Emissions are
 * x . ctc.w[id] + ctc.b[id] - log-sum-exp of the row, formed for the blank and the tokens asked for only (pfhip_op_ctc_emissions);
 * the path is the Viterbi optimum of pfhip_op_ctc_align, whose comment states the recurrence and the tie rule.
 * tok_begin / tok_end [batch][max_tokens]: the first row of token j on that path and one past its last, in tok_frame's numbering
 * (rows of the utterance with the prompt rows counted, so >= 4); tok_logp (may be NULL): the token's emission at tok_begin;
 * score [batch] (may be NULL): the path's log-probability.  An utterance too short for its tokens (rows < tokens + equal neighbours;
 * an utterance of fewer than 400 samples has no rows) has score -inf and -1 in every span; the others are served.
 * PFHIP_ERR_ARG, before any launch: a token outside 0 .. vocab - 1 or equal to the blank, a negative count, a batch mismatch, no
 * previous forward of this thread on this handle.  PFHIP_ERR_UNSUPPORTED: a Paraformer handle.  PFHIP_ERR_CAPACITY: max_tokens below
 * the longest n_tokens.  The forward itself is unchanged by this: it only keeps the row log-sum-exp both heads form anyway. */
typedef struct pfhip_svs_align_out { int32_t* tok_begin; int32_t* tok_end; float* tok_logp; float* score; int max_tokens; } pfhip_svs_align_out;
pfhip_status pfhip_svs_align(pfhip_model* m, const int32_t* const* tokens, const int* n_tokens, int batch, pfhip_svs_align_out* out);
/* pfhip_svs_forward[_s16] and the alignment of its own GREEDY tokens in ONE call: with spans != NULL each utterance's text tokens (its
 * kept ids behind the four tags, ids[b][4:]) are aligned against its own speech rows inside the forward's stream work — a plan kernel
 * turns the collapse's counts into the alignment's sizes on the device (pfhip_op_ctc_greedy_plan), then the two kernels of
 * pfhip_svs_align — and the spans travel in the forward's one device-to-host copy, before its one synchronise: no second upload,
 * copy or synchronise.  What comes back in `out` is that of pfhip_svs_forward bit for bit, and what comes back in `spans` is that of
 * pfhip_svs_align(ids[b][4:]) after it bit for bit (same rows, same kernels); after a range-guard re-run both belong to the re-run.
 * spans->max_tokens counts the tokens BEHIND the tags (PFHIP_ERR_CAPACITY below the longest token_num[b] - 4); tok_begin / tok_end are
 * required, tok_logp / score may be NULL.  spans == NULL: pfhip_svs_forward itself, which launches what it always launched.
 * The emissions and back-pointers are sized before the launch from n_lab[b] <= N_b (a kept token needs a frame): sum_b N_b (N_b + 1)
 * floats over the batch's speech rows N_b, capped at PFHIP_SVS_SPAN_MAX_FLOATS (96 utterances of 30 s need 24 M; the back-pointers
 * take two bytes per float on top).  An utterance whose emissions would end beyond the cap is answered as an infeasible one — spans
 * -1, score -inf — and the others are served; align it with pfhip_svs_align, or in a smaller batch. */
#define PFHIP_SVS_SPAN_MAX_FLOATS ((size_t)64 << 20)
pfhip_status pfhip_svs_forward_spans(pfhip_model* m, const float* const* pcm, const int* n_samples, int batch, const int32_t* lid,
                                     const int32_t* textnorm, pfhip_svs_out* out, pfhip_svs_align_out* spans);
pfhip_status pfhip_svs_forward_spans_s16(pfhip_model* m, const int16_t* const* pcm, const int* n_samples, int batch, const int32_t* lid,
                                         const int32_t* textnorm, pfhip_svs_out* out, pfhip_svs_align_out* spans);

/* ---- hotword context graph of the CTC prefix beam search (ctx_graph.cpp; host only, no device) ----
 * What CtcPrefixDecoder::LoadHwsRes builds through ContextGraph::BuildContextGraph and walks with GetNextState
 * (onnxruntime/src/context_graph.cpp:33-118), as a deterministic trie from state 0.  Hotword j is the token ids
 * ids[sum n_ids[..j] .. + n_ids[j]) with one weight per token, tok_weight likewise packed (the reference's weight of a token is
 * hotword score x UTF-8 length of its string, :76-77: the caller's product).  With minCum(node) = the least cumulative weight over
 * the hotwords through a node:
 *   - the arc into a node weighs minCum(node) - minCum(parent); the last token of a hotword leads back to state 0 and weighs the
 *     hotword's cumulative weight - minCum(parent) (of duplicates the least);
 *   - a token that matches no arc of an inner state scores the escape weight -minCum(state) and leads to state 0 — it is NOT tried
 *     again from state 0 (reference behaviour); from state 0 a miss scores 0;
 *   - a hotword that is a proper prefix of another: the node it ends on stays (the longer one goes on from it), is final, counts the
 *     shorter word in its minCum, carries state 0's arcs as well (each heavier by the shorter word's cumulative weight - minCum; an
 *     arc of its own with the same label wins) and keeps its escape weight, so a miss there takes the shorter word's bonus away.
 * Arcs of a state are sorted by label.  PFHIP_ERR_ARG: an id outside 1 .. vocab - 1 (0 is the escape label), an empty word, a
 * non-finite weight or cumulative weight, a NULL argument; pfhip_op_ctc_prefix_beam therefore only ever sees validated indices.
 * pfhip_ctx_graph_dump (tests): *n_states / *n_arcs always; with every array given, the CSR form — arc_begin [cap_states + 1],
 * escape [cap_states], arc_label / arc_next / arc_weight [cap_arcs] — or PFHIP_ERR_CAPACITY where a cap is too small.
 * The reference's slip of the score index after a skipped over-long hotword (:56-61) has no counterpart: weights arrive per token. */
typedef struct pfhip_ctx_graph pfhip_ctx_graph;
pfhip_status pfhip_ctx_graph_create(const int32_t* ids, const int* n_ids, const float* tok_weight, int n_words, int vocab,
                                    pfhip_ctx_graph** g);
void pfhip_ctx_graph_destroy(pfhip_ctx_graph* g);
int pfhip_ctx_graph_vocab(const pfhip_ctx_graph* g);
pfhip_status pfhip_ctx_graph_dump(const pfhip_ctx_graph* g, int* n_states, int* n_arcs, int32_t* arc_begin, float* escape, int cap_states,
                                  int32_t* arc_label, int32_t* arc_next, float* arc_weight, int cap_arcs);

/* ---- token n-gram language model of the device searches (lm_graph.cpp; host only, no device) ----
 * A back-off n-gram model over the MODEL'S OWN TOKENS (characters or BPE pieces), as SRILM writes it in ARPA form, for shallow
 * fusion inside the device searches and for rescoring (pfhip_op_lm_score, pfhip_ops.h).  It is NOT the reference's TLG.fst route
 * (InitLm): a word-level model needs a lexicon transducer, and BiasLm walks that same WFST; both stay outside this library.
 * Labels: 0 .. vocab - 1 are token ids, vocab is </s>, vocab + 1 is <s>, vocab + 2 is <unk>.  <s> appears inside histories only: an
 * n-gram of length >= 2 that predicts <s> is dropped, the unigram <s> gives the state of the history (<s>) and no arc.  <unk> may
 * only be a unigram (PFHIP_ERR_ARG above order 1) and gives no state.  An n-gram of length >= 2 whose history (its first n - 1
 * labels) is not itself a kept n-gram is dropped.
 * pfhip_lm_graph_create: n-grams of length n = 1 .. order (order <= PFHIP_LM_ORDER_MAX), n_grams[n - 1] of each, packed by
 * length: labels holds n labels per n-gram (oldest first, the predicted label last), log10_prob / log10_backoff one value per
 * n-gram in the same sequence (back-off 0 where ARPA gives none; the back-off of a highest-order n-gram is not read).
 * The automaton:
 *   - state 0 is the empty history; every kept n-gram of length 1 .. order - 1 is a state; states are numbered by history length,
 *     then lexicographically by labels, oldest label first;
 *   - state h has one arc per kept n-gram (h, w), sorted by label w; the arc's next state is the longest suffix of (h, w) that is a
 *     state (0 if none);
 *   - each state has a back-off weight and a back-off state: the longest PROPER suffix of h that is a state (0 if none), always a
 *     strictly shorter history, so a chain of back-offs ends in state 0 after at most order - 1 steps;
 *   - state 0 is direct-indexed by label: uni_w / uni_next [vocab + 1].  A token without a unigram scores <unk>'s unigram where
 *     there is one, else oov_log10, and leads to state 0.  uni_w[vocab] is only meaningful when has_eos (</s> has a unigram);
 *   - the start state is the state of the history (<s>) if it exists, else 0.
 * A step from state s by label w: in state 0 add uni_w[w] and go to uni_next[w]; elsewhere take the arc of s with label w (add its
 * weight, go to its next state), or add the back-off weight, fall to the back-off state and try again.
 * Weights are natural logarithms with the scale and the bonus baked in, so that a search only ever adds: an arc (and a uni_w entry)
 * is fl32((p10 * ln10) * scale + token_bonus), without the bonus where the label is </s>; a back-off weight is
 * fl32((b10 * ln10) * scale); ln10 = 2.302585092994046, every operation an IEEE double operation on its own, one rounding to float.
 * PFHIP_ERR_ARG with a pfhip_last_error text: order outside 1 .. PFHIP_LM_ORDER_MAX, a negative count, sizes beyond int32 indices,
 * a label outside 0 .. vocab + 2, an n-gram listed twice, a non-finite number or a weight that is not finite in fp32.
 * pfhip_lm_graph_create_from_arpa reads an ARPA file and feeds the entry above.  tokens [vocab]: the model's token strings, UTF-8; a
 * word is the token id whose string it equals byte for byte (the lowest id among duplicates); <s>, </s> and <unk> are recognised by
 * name first.  An n-gram with any other unknown word, or with <unk> above order 1, is skipped and counted in *n_skipped (optional).
 * Numbers are read with strtod.  PFHIP_ERR_ARG with a text: the file cannot be read, no \data\ or \end\ line, a section missing or
 * out of turn, a count that disagrees with its section, a line with the wrong number of fields, a non-finite or malformed number,
 * an order above the cap, counts beyond int32 indices.
 * pfhip_lm_graph_dump (tests): the four counts always; with every array given — uni_w / uni_next [cap_uni >= vocab + 1], arc_begin
 * [cap_states + 1] (arc_begin[0] == arc_begin[1] == 0: state 0 keeps its arcs in uni_*), backoff_w / backoff_state [cap_states],
 * arc_label / arc_next / arc_weight [cap_arcs] — the arrays, or PFHIP_ERR_CAPACITY where a cap is too small. */
#define PFHIP_LM_ORDER_MAX 6
typedef struct pfhip_lm_graph pfhip_lm_graph;
/* pfhip_set_token_lm: the model every SEARCH of this handle's forwards walks from now on (shallow fusion; pfhip_ops.h states the
 * recurrences): pfhip_svs_forward_beam[_s16], pfhip_svs_forward_beam_sets[_s16], merged beam callers (pfhip_svs_set_beam_merging)
 * and pfhip_offline_forward_bias[_s16] then run the searches' model-walking instantiations.  `score` is the total including the
 * model's share, ctc_score / am_score and ctx_score keep their meaning, and the share itself is read with pfhip_get_tensor
 * "beam_lm_score": [batch][stride] laid out as the call's own score array (0 behind n_hyp), the calling thread's last searching
 * forward, with the lifetime rule of "ctc_topk_*" (until the execution context runs another forward).  `out`, the detail buffers
 * and the spans stay bit for bit the plain call's; a range-guard re-run redoes the search with the model.  Greedy calls do not read
 * the model.  The packed image is copied to the handle's device once, into memory the handle owns: the host graph may be destroyed
 * afterwards.  NULL removes the model; with none set every call launches exactly what it launched before.
 * PFHIP_ERR_ARG: a graph of another vocabulary, a forward in flight, a handle that is not the one pfhip_create returned.
 * PFHIP_ERR_UNSUPPORTED: a multi-device group.  This is not InitLm: a TLG.fst is still not read (see above). */
pfhip_status pfhip_set_token_lm(pfhip_model* m, const pfhip_lm_graph* lm);
pfhip_status pfhip_lm_graph_create(int order, const int* n_grams, const int32_t* labels, const double* log10_prob,
                                   const double* log10_backoff, int vocab, float scale, float token_bonus, float oov_log10,
                                   pfhip_lm_graph** g);
pfhip_status pfhip_lm_graph_create_from_arpa(const char* path, const char* const* tokens, int vocab, float scale, float token_bonus,
                                             float oov_log10, pfhip_lm_graph** g, long long* n_skipped);
void pfhip_lm_graph_destroy(pfhip_lm_graph* g);
int pfhip_lm_graph_vocab(const pfhip_lm_graph* g);
int pfhip_lm_graph_order(const pfhip_lm_graph* g);
pfhip_status pfhip_lm_graph_dump(const pfhip_lm_graph* g, int* n_states, int* n_arcs, int* start, int* has_eos, float* uni_w,
                                 int32_t* uni_next, int cap_uni, int32_t* arc_begin, float* backoff_w, int32_t* backoff_state,
                                 int cap_states, int32_t* arc_label, int32_t* arc_next, float* arc_weight, int cap_arcs);

/* pfhip_svs_forward[_s16] with the CTC prefix beam search — and, through a context graph, hotwords — behind its head: what the
 * reference's servers run for this model through a CtcPrefixDecoder per connection (funasrruntime.cpp:836-894,
 * sensevoice-small.cpp:651-657, ctc-prefix-decoder.cpp:157-299).  The head runs ONCE, in its top-k form with k = first_beam
 * (pfhip_op_ctc_head_topk: no logits matrix), the search (pfhip_op_ctc_prefix_beam, which states the recurrence and the tie rule)
 * runs over the SPEECH rows of every utterance — the four prompt rows are no CTC rows (sensevoice-small.cpp:422) — and its results
 * travel in the forward's one device-to-host copy, before its one synchronise.  `out` comes back as pfhip_svs_forward's bit for bit;
 * pfhip_svs_align afterwards works against the same rows (e.g. on ids[b][0]); after a range-guard re-run everything belongs to the
 * re-run, whose k best columns come from the unfused head's rows.
 * opts: 1 <= first_beam, second_beam <= 16, 1 <= nbest <= second_beam, graph NULL or built for this model's vocabulary (it must
 * stay alive for the call).  beam, caller-owned: n_hyp [batch]; ids [batch][nbest][max_tokens] (text tokens only, no tags; written
 * up to n_tokens); n_tokens [batch][nbest] — the TRUE length; score / ctc_score / ctx_score [batch][nbest] (may be NULL).  An
 * utterance without rows has n_hyp 0.  PFHIP_ERR_CAPACITY where max_tokens is below the longest returned hypothesis: n_hyp,
 * n_tokens and the scores are written all the same, so n_tokens carries the length needed.  PFHIP_ERR_UNSUPPORTED: a Paraformer
 * handle.  PFHIP_ERR_ARG: beams outside 1..16, nbest outside 1..second_beam, a graph of another vocabulary, a missing buffer.
 * With pfhip_svs_set_batching on, the call is served alone, past the merge queue, unless pfhip_svs_set_beam_merging is on (below).
 * pfhip_get_tensor "ctc_topk_ids" (int32 words) / "ctc_topk_logp": the [M][first_beam] columns the search read, prompt rows
 * included. */
typedef struct pfhip_svs_beam_opts { int first_beam; int second_beam; int nbest; const pfhip_ctx_graph* graph; } pfhip_svs_beam_opts;
typedef struct pfhip_svs_beam_out {
  int32_t* n_hyp; int32_t* ids; int32_t* n_tokens; float* score; float* ctc_score; float* ctx_score; int max_tokens;
} pfhip_svs_beam_out;
pfhip_status pfhip_svs_forward_beam(pfhip_model* m, const float* const* pcm, const int* n_samples, int batch, const int32_t* lid,
                                    const int32_t* textnorm, pfhip_svs_out* out, const pfhip_svs_beam_opts* opts, pfhip_svs_beam_out* beam);
pfhip_status pfhip_svs_forward_beam_s16(pfhip_model* m, const int16_t* const* pcm, const int* n_samples, int batch, const int32_t* lid,
                                        const int32_t* textnorm, pfhip_svs_out* out, const pfhip_svs_beam_opts* opts,
                                        pfhip_svs_beam_out* beam);
/* One call, several searches: pfhip_svs_forward_beam with every utterance on its own set of options — the sibling of
 * pfhip_offline_forward_hwsets for the CTC model (one connection, one CtcPrefixDecoder with its own hotwords: websocket-server.cpp:173).
 * sets [n_sets]; set_of [batch] names each utterance's set, -1: no search for it (n_hyp 0).  The head runs ONCE in its top-k form
 * with k = the largest first_beam among the sets in use (no set in use: the greedy head of pfhip_svs_forward), and ONE search launch
 * serves all utterances (pfhip_op_ctc_prefix_beam_multi): utterance b reads the first first_beam columns of its rows, which are the
 * columns a head run at k = first_beam leaves, bit for bit (the value and order rules of pfhip_op_ctc_head_topk do not depend on
 * k), so with every utterance on one set the call equals pfhip_svs_forward_beam bit for bit, and `out` is pfhip_svs_forward's.
 * Results cross in the forward's one copy, before its one synchronise; a range-guard re-run redoes all of it.
 * beam: as above with nbest stride = the largest nbest among the sets in use (1 if none): ids [batch][stride][max_tokens], the
 * others [batch][stride]; slots from an utterance's own nbest on read as slots behind n_hyp.  Errors are pfhip_svs_forward_beam's,
 * per set in use; PFHIP_ERR_ARG also for n_sets < 1 or a set_of outside -1 .. n_sets - 1.
 * pfhip_get_tensor "ctc_topk_*" after it: [rows][k] with that k (pfhip_debug_poke "svs_topk_k").
 * The graphs of this call and of merged beam callers stay on the device: a per-device bank of packed graph images shared by the
 * execution contexts and found again by content (hash + byte compare).  A graph seen before costs no upload; all misses of a forward
 * go up in one copy; least recently used graphs are evicted, never one a forward in flight uses; a graph the bank cannot take goes
 * up with the call.  pfhip_svs_set_graph_bank_bytes bounds it (default PFHIP_CTX_GRAPH_BANK_MB = 16 per device; 0 banks nothing;
 * set it while no forward is in flight, PFHIP_ERR_ARG otherwise).  Results do not depend on the bank.  pfhip_svs_forward_beam
 * served alone keeps uploading its graph with the call. */
pfhip_status pfhip_svs_forward_beam_sets(pfhip_model* m, const float* const* pcm, const int* n_samples, int batch, const int32_t* lid,
                                         const int32_t* textnorm, pfhip_svs_out* out, const pfhip_svs_beam_opts* sets, int n_sets,
                                         const int32_t* set_of, pfhip_svs_beam_out* beam);
pfhip_status pfhip_svs_forward_beam_sets_s16(pfhip_model* m, const int16_t* const* pcm, const int* n_samples, int batch,
                                             const int32_t* lid, const int32_t* textnorm, pfhip_svs_out* out,
                                             const pfhip_svs_beam_opts* sets, int n_sets, const int32_t* set_of, pfhip_svs_beam_out* beam);
pfhip_status pfhip_svs_set_graph_bank_bytes(pfhip_model* m, int64_t bytes);
/* Totals over the handle's device: graphs found resident, uploaded, dropped for room, refused (served from the call's workspace). */
typedef struct pfhip_svs_graph_bank_stats_t {
  int64_t hits, misses, evictions, refused;
  int64_t bytes_in_use, bytes_capacity, graphs_resident;
} pfhip_svs_graph_bank_stats_t;
pfhip_status pfhip_svs_graph_bank_stats(pfhip_model* m, pfhip_svs_graph_bank_stats_t* out);
/* Beam callers in the merge queue (pfhip_svs_set_batching): on != 0 lets concurrent pfhip_svs_forward_beam[_s16] and
 * pfhip_svs_forward_beam_sets[_s16] callers share packed forwards with each other and with greedy callers of the same sample
 * format: one head launch at the largest first_beam, one search launch with every utterance on its caller's beams and graph (graphs
 * de-duplicated by pointer, then by content), each caller dealt its hypotheses at its own nbest stride and max_tokens.  A caller
 * whose max_tokens is too small fails alone with PFHIP_ERR_CAPACITY, n_hyp / n_tokens / scores written as in the lone call.  Off
 * (the default), every beam call is a forward of its own, as before.  Merged, `out` is that of a separate call as far as
 * pfhip_svs_set_batching states it, and the hypotheses are the search's on the columns of the forward that served the caller:
 * pfhip_get_tensor "ctc_topk_ids" / "ctc_topk_logp" then return the CALLING THREAD's own utterances' rows [own rows][k] (the
 * lifetime rule of pfhip_svs_align), and pfhip_debug_poke "svs_topk_k" that forward's k. */
pfhip_status pfhip_svs_set_beam_merging(pfhip_model* m, int on);

/* ---- hotwords for any Paraformer: a biased beam search over the head's candidates (extension) --------
 * The reference biases a Paraformer two ways: the contextual checkpoint (model_eb.onnx + bias decoder), and BiasLm inside the WFST
 * search, which needs a TLG.fst.  Without an LM its Paraformer::Forward never looks at the connection's CtcPrefixDecoder
 * (paraformer.cpp:563-579), so a client's hotwords are dropped.  This is NOT either of those paths: the head's k best columns of
 * every token row (topk.hip) are searched on the device with a context graph (pfhip_op_nbest_ctx_beam, include/pfhip_ops.h, states
 * the recurrence and the tie rule).  A Paraformer's token rows are independent positions, so the search replaces tokens position by
 * position and never changes the token count: n_fires, token_num, fire frames and head timestamps of the same forward stay valid
 * for the biased ids.  It works on any Paraformer (plain, small, contextual: both biases at once) and has not been evaluated on
 * real speech.
 * pfhip_offline_forward_bias[_s16] is pfhip_offline_forward_detail[_s16] plus the search: `out` and `det` (may be NULL) come back
 * bit for bit as that call's with the same det.  sets [n_sets]: 1 <= width <= 8 (and <= vocab), 1 <= nbest <= beam <= 16, graph
 * NULL or built for this model's vocabulary (alive for the call; it goes up with the call).  set_of [batch] names each utterance's
 * set, -1: no search for it (n_hyp 0); NULL: every utterance on set 0.  The head runs ONCE in its top-k form at k = the largest of
 * the widths in use and det->nbest_k; an utterance reads the first `width` columns of its rows (the value and order rules of the
 * head do not depend on k).  The search covers min(token_num[b], n_fires[b]) rows, read from the device's own counts on the
 * forward's stream, and its results cross before the forward's one synchronise; after a range-guard re-run everything belongs to
 * the re-run; each execution context (pfhip_set_inflight) owns its buffers.  With pfhip_set_batching on the call is served alone,
 * past the merge queue.
 * bias_out, caller-owned, with stride = the largest nbest among the sets in use (1 if none): n_hyp [batch]; ids
 * [batch][stride][max_tokens] (written up to n_tokens); n_tokens [batch][stride] = the searched row count for a live hypothesis;
 * score (am + ctx) / am_score / ctx_score [batch][stride] (may be NULL; -inf / -inf / 0 behind n_hyp).  Without a graph hypothesis
 * 0 is the greedy sequence.  PFHIP_ERR_UNSUPPORTED: a SenseVoice handle, a multi-device group.  PFHIP_ERR_CAPACITY where
 * bias_out->max_tokens is below the longest returned hypothesis: n_hyp, n_tokens and the scores are written all the same.
 * PFHIP_ERR_ARG: a limit broken in a set in use, n_sets < 1, a set_of outside -1 .. n_sets - 1, a missing buffer, a graph of
 * another vocabulary. */
typedef struct pfhip_bias_opts { int width; int beam; int nbest; const pfhip_ctx_graph* graph; } pfhip_bias_opts;
typedef struct pfhip_bias_out {
  int32_t* n_hyp; int32_t* ids; int32_t* n_tokens; float* score; float* am_score; float* ctx_score; int max_tokens;
} pfhip_bias_out;
pfhip_status pfhip_offline_forward_bias(pfhip_model* m, const float* const* pcm, const int* n_samples, int batch, int sample_rate,
                                        const float* const* hw_emb, const int* n_hotwords, int n_hw_sets, const int* hw_set_of,
                                        pfhip_out* out, const pfhip_detail* det, const pfhip_bias_opts* sets, int n_sets,
                                        const int32_t* set_of, pfhip_bias_out* bias_out);
pfhip_status pfhip_offline_forward_bias_s16(pfhip_model* m, const int16_t* const* pcm, const int* n_samples, int batch, int sample_rate,
                                            const float* const* hw_emb, const int* n_hotwords, int n_hw_sets, const int* hw_set_of,
                                            pfhip_out* out, const pfhip_detail* det, const pfhip_bias_opts* sets, int n_sets,
                                            const int32_t* set_of, pfhip_bias_out* bias_out);

/* ---- inspection (parity tests) -----------------------------------------------------------------
 * Copies a named intermediate of the LAST forward to host: "feats" [M,560], "enc" [M,d],
 * "alphas" [M] (without the tail slot), "emb" [sum fires, d], "logp" [sum fires, vocab],
 * "fire_frame" [sum fires] (the fire frames of a forward that recorded them, as floats: the values are small integers).
 * Rows are utterance-major in batch order.  *n_out = floats written.  A SenseVoice handle has "feats" [M,560] (prompt rows
 * included, M = sum of T + 4), "enc" [M,d] (the rows after tp.norm, which the CTC head reads) and "lse" [M] (the log-sum-exp of
 * every row's logits as the CTC head that ran kept it: what pfhip_svs_align subtracts). */
pfhip_status pfhip_get_tensor(pfhip_model* m, const char* name, float* dst, size_t cap_floats,
                              size_t* n_out);

/* ---- per-kernel timing (bench.py roofline leg) -------------------------------------------------
 * When enabled, each launch of a kernel class is bracketed by hipEvents on the launch stream.
 * `on`: 0 = off, 1 = every class, any other value = bit mask of classes (bit c = class c; bench.py times only
 * the dominant class, 1<<0 | 1<<8 ... see below, so that the event records do not perturb the timed region).
 * Classes: 0 gemm, 1 attention, 2 layernorm, 3 fsmn, 4 fbank, 5 cif, 6 head(log-softmax/argmax), 7 other. */
#define PFHIP_NUM_KCLASS 8
typedef struct {
  double ms[PFHIP_NUM_KCLASS];       /* summed device time                                         */
  int64_t launches[PFHIP_NUM_KCLASS];
  double flops[PFHIP_NUM_KCLASS];    /* algorithmic flops issued (pad rows/cols excluded)           */
  double bytes[PFHIP_NUM_KCLASS];    /* algorithmic bytes (compulsory reads + writes)               */
} pfhip_profile;
/* ---- in-process multi-GPU: one handle, one replica per device (replicas only, no collective) -----------------
 * The reference server holds ONE model handle that all `decoder-thread-num` threads call into (funasr-wss-server.cpp:479-481,
 * websocket-server.cpp:387-403).  A group keeps that shape on a multi-GPU node: the handle returned is replica 0, further
 * replicas (full copies of the weights) live on the other devices; pfhip_offline_forward routes each call (or each merged
 * batch, pfhip_set_batching) to the replica with the fewest calls in flight, pfhip_stream_create pins a new connection to the
 * replica with the fewest open streams for its lifetime (device-resident caches), pfhip_set_hotwords / pfhip_set_batching /
 * pfhip_set_stream_batching apply to every replica.  Results do not depend on which replica served a call.  No data moves
 * between devices.  For several forwards in flight on ONE device use pfhip_set_inflight (contexts share the weights); listing a
 * device twice here still works but builds a second full copy of the weights there.
 * PFHIP_DEVICES="0,1,..." in the environment makes pfhip_create / pfhip_create_from_memory build such a group (their `device`
 * argument is then ignored), so the stock server needs no code change to use every GPU of the node.
 * pfhip_offline_enqueue / pfhip_offline_fetch (device pointers) always use replica 0.  pfhip_group_stats counts per replica
 * (its contexts included); pfhip_inflight_stats per execution slot. */
pfhip_status pfhip_create_group(const void* blob, size_t blob_bytes, const char* manifest_json, const int* devices, int n_devices,
                                pfhip_model** out);
int pfhip_group_size(const pfhip_model* m);
/* Per replica (arrays of at least pfhip_group_size entries, any may be NULL): device ordinal, offline calls and utterances
 * served so far, streams open now. */
pfhip_status pfhip_group_stats(pfhip_model* m, int* devices, int64_t* calls, int64_t* utterances, int* open_streams, int cap);

/* Test hook, not part of the serving path: "blstm_flag" (value != 0) raises the timestamp head's error word for the next
 * timestamp request only — as a step-barrier time-out of the persistent BLSTM kernel would — which then has to be served by the
 * per-step recurrence; "blstm_fallbacks" returns (as the status value) how many requests were served that way; "plane_forwards"
 * how many forwards of this context ran the encoder on plane-image operands (gemm_p3.hip: batches of PFHIP_PLANES_MIN_ROWS+ rows);
 * "format_splits" how many merged batches (pfhip_set_batching) were cut short because f32 and s16 callers were queued together;
 * "ctc_unfused" (value != 0) sends the next pfhip_svs_forward of EVERY execution context of the handle through the unfused CTC head
 * (once each: with pfhip_set_inflight(1) that is the next forward); "ctc_unfused_forwards" returns how many forwards took that head,
 * summed over the contexts; "ctc_head_chunks" how many row chunks the unfused head of the calling thread's last forward ran;
 * "svs_span_cap" (value floats, 0 = back to the constant) stands in for PFHIP_SVS_SPAN_MAX_FLOATS on every context of the handle;
 * "svs_unfused_rows" how many rows went through the unfused head chunks in the forward — lone or merged — that served the calling
 * thread's last pfhip_svs_forward[_spans] (a merged forward sends only the rows of the callers who asked for log-prob rows), and
 * "svs_forward_calls" how many callers that forward served (1: a lone caller). */
pfhip_status pfhip_debug_poke(pfhip_model* m, const char* what, int value);
pfhip_status pfhip_profile_enable(pfhip_model* m, int on);
pfhip_status pfhip_profile_read(pfhip_model* m, pfhip_profile* out, int reset);

/* ---- Speech quality: the DNSMOS networks (utils/dnsmos_local.py; an extension of scope) ----
 *   pfhip_mos_create_from_files  <-> ComputeScore.__init__ (dnsmos_local.py:25-27): primary_onnx = utils/DNSMOS/sig_bak_ovr.onnx or
 *                                utils/pDNSMOS/sig_bak_ovr.onnx, p808_onnx_or_null = utils/DNSMOS/model_v8.onnx (NULL: the p808 fields
 *                                are NaN).  The graphs are walked node by node and every kernel, bias and constant is taken from the
 *                                file; a graph that is not of this family is PFHIP_ERR_FORMAT with pfhip_last_error naming the first
 *                                node that does not fit (the sig.onnx / bak_ovr.onnx variants are refused so).
 *   pfhip_mos_create_from_memory a container of kind "dnsmos" (convert.py convert_dnsmos, or pfhip_read_model_files(kind "dnsmos",
 *                                model = primary, second = p808) — the same bytes).  Weights are packed once here; a convolution
 *                                weight that is not finite or leaves the fp16 two-plane range is PFHIP_ERR_UNSUPPORTED.
 *   pfhip_mos_score[_s16]        <-> ComputeScore.__call__ (dnsmos_local.py:51-104) for n_clips clips of 16 kHz audio (f32 in [-1, 1] or
 *                                16-bit PCM standing for s / 32768.f, bit for bit equal): a clip shorter than 144160 samples is
 *                                appended to itself until it is not; num_hops = int(floor(len / 16000) - 9.01) + 1; window idx is
 *                                [int(idx * 16000), int((idx + 9.01) * 16000)) in double, skipped where that is shorter than 144160;
 *                                the raw P.835 outputs go through get_polyfit_val (plain or personalized); everything is averaged over
 *                                the scored windows, on the host in double.  An empty clip is PFHIP_ERR_ARG.  Other sample rates go
 *                                through pfhip_resample first (Kaldi's resampler, where the script calls librosa's).
 *   pfhip_mos_score_windows[_s16] the per-window raw outputs behind that: raw [n_windows][4] = (p808, sig, bak, ovr), clip after clip,
 *                                num_hops / n_scored [n_clips]; *n_windows is always set, PFHIP_ERR_CAPACITY above cap_windows.
 *   pfhip_mos_set_workspace      the cap in bytes on the activations of one slab of windows (default 2 GiB; one window always runs).
 *                                Results do not depend on it, nor on what else a call holds.
 * A handle serves one call at a time (calls on one handle are serialised); pfhip_mos_destroy waits for the device first. */
typedef struct pfhip_mos pfhip_mos;
typedef struct {
  int32_t num_hops, n_scored;
  double p808, sig_raw, bak_raw, ovr_raw, sig, bak, ovr;
} pfhip_mos_result;
pfhip_status pfhip_mos_create_from_files(const char* primary_onnx, const char* p808_onnx_or_null, int device, pfhip_mos** out);
pfhip_status pfhip_mos_create_from_memory(const void* blob, size_t blob_bytes, const char* manifest_json, int device, pfhip_mos** out);
void pfhip_mos_destroy(pfhip_mos* h);
pfhip_status pfhip_mos_set_workspace(pfhip_mos* h, size_t bytes);
pfhip_status pfhip_mos_score(pfhip_mos* h, const float* const* pcm, const int64_t* n_samples, int n_clips, int personalized,
                             pfhip_mos_result* results);
pfhip_status pfhip_mos_score_s16(pfhip_mos* h, const int16_t* const* pcm, const int64_t* n_samples, int n_clips, int personalized,
                                 pfhip_mos_result* results);
pfhip_status pfhip_mos_score_windows(pfhip_mos* h, const float* const* pcm, const int64_t* n_samples, int n_clips, int32_t* num_hops,
                                     int32_t* n_scored, float* raw, size_t cap_windows, size_t* n_windows);
pfhip_status pfhip_mos_score_windows_s16(pfhip_mos* h, const int16_t* const* pcm, const int64_t* n_samples, int n_clips, int32_t* num_hops,
                                         int32_t* n_scored, float* raw, size_t cap_windows, size_t* n_windows);

#ifdef __cplusplus
}
#endif
#endif /* PFHIP_H_ */
