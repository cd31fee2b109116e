// The offline slice of the reference's handle API (onnxruntime/include/funasrruntime.h:69-115), same names, argument
// meaning and error behaviour, on top of the HIP plug-ins — what the websocket server's decoder threads call
// (websocket/bin/websocket-server.cpp:81-89,173,209-210):
//
//   FunOfflineInit          funasrruntime.cpp:36-40     OfflineStream: VAD + acoustic model (+ batch size)
//   FunOfflineInferBuffer   funasrruntime.cpp:208-337   LoadPcmwav -> CutSplit -> FetchDynamic -> Model::Forward -> re-ordering
//   FunASRGetResult / FunASRGetStamp / FunASRGetRetSnippetTime / FunASRFreeResult   funasrruntime.cpp:540-640
//   CompileHotwordEmbedding funasrruntime.cpp:862-867
//   FunOfflineUninit        funasrruntime.cpp:806-814
//
// Stand-alone mirror: inside the reference tree the real funasrruntime.cpp stays and only the Model classes are swapped
// (INTEGRATION.md).  With PUNC_DIR given the text goes through CTTransformerHip::AddPunc like the reference's punc_handle
// (funasrruntime.cpp:317-320).  What is NOT here: audio container decode (ffmpeg), ITN (WFST text normaliser) and sentence
// stamps — text handling above the hot path.  Result text = the vocabulary strings of the greedy tokens (or space-separated ids without
// a tokens.json); stamps have the reference's "[[b,e],[b,e]...]" millisecond format.
#pragma once
#include <map>
#include <string>
#include <unordered_map>
#include <vector>

#define MODEL_SVS "SenseVoiceSmall"    // com-define.h:41: a MODEL_DIR whose name contains it holds that model (offline-stream.cpp:50-56)
#define MODEL_DIR "model-dir"          // com-define.h:14-28 keys of the model_path map
#define OFFLINE_MODEL_DIR "model-dir"
#define ONLINE_MODEL_DIR "online-model-dir"
#define VAD_DIR "vad-dir"
#define PUNC_DIR "punc-dir"
#define LM_DIR "lm-dir"                // com-define.h:18; its files: TLG.fst, config.yaml, lexicon.txt (:70, :86-87)
#define LM_FST_RES "TLG.fst"
#define LM_CONFIG_NAME "config.yaml"
#define LEX_PATH "lexicon.txt"
#define QUANTIZE "quantize"
#define VAD_QUANT "vad-quant"
#define PUNC_QUANT "punc-quant"
#define TOKEN_PATH_KEY "token-path"    // (not a key of the reference: an optional override of <model-dir>/tokens.json for harness runs)
// com-define.h:52-88 file names inside those directories
#define MODEL_NAME "model.onnx"
#define QUANT_MODEL_NAME "model_quant.onnx"
#define MODEL_EB_NAME "model_eb.onnx"
#define TORCH_MODEL_NAME "model.torchscript"
#define TORCH_MODEL_EB_NAME "model_eb.torchscript"
#define ENCODER_NAME "model.onnx"
#define QUANT_ENCODER_NAME "model_quant.onnx"
#define DECODER_NAME "decoder.onnx"
#define QUANT_DECODER_NAME "decoder_quant.onnx"
#define AM_CMVN_NAME "am.mvn"
#define AM_CONFIG_NAME "config.yaml"
#define VAD_CMVN_NAME "am.mvn"
#define VAD_CONFIG_NAME "config.yaml"
#define MODEL_SEG_DICT "seg_dict"
#define TOKEN_PATH "tokens.json"

typedef void* FUNASR_HANDLE;
typedef void* FUNASR_RESULT;
typedef void* FUNASR_DEC_HANDLE;
typedef enum { RASR_NONE = -1, RASRM_CTC_GREEDY_SEARCH = 0 } FUNASR_MODE;      // funasrruntime.h:30-35 (subset)
typedef enum { ASR_OFFLINE = 0, ASR_ONLINE = 1, ASR_TWO_PASS = 2 } ASR_TYPE;   // funasrruntime.h:48-52
typedef void (*QM_CALLBACK)(int cur_step, int n_total);

// model_path as the reference's servers fill it (funasr-wss-server.cpp:203-320): MODEL_DIR / VAD_DIR / PUNC_DIR are directories in
// the reference's layout (model.onnx | model_quant.onnx with QUANTIZE = "true" | model.torchscript with use_gpu, model_eb.onnx,
// seg_dict, am.mvn, config.yaml, tokens.json); the constructor makes the calls of OfflineStream::OfflineStream
// (offline-stream.cpp:4-129) on the HIP plug-ins.  A directory that holds a converted container (x.pfhip.{bin,json}) instead of
// ONNX files works too.  A model that fails to load ends the process like the reference (paraformer.cpp:43-46).
// A MODEL_DIR whose name contains MODEL_SVS gets SenseVoiceSmallHip instead of ParaformerHip, as offline-stream.cpp:50-56 picks the
// model; FunOfflineInferBuffer then routes by model type as funasrruntime.cpp:265-266 does, with its two trailing parameters
// svs_lang / svs_itn (funasrruntime.h:107), and ignores hw_emb for that model, as the reference does.
FUNASR_HANDLE FunOfflineInit(std::map<std::string, std::string>& model_path, int thread_num, bool use_gpu = true,
                             int batch_size = 1);
// sz_buf: n_len BYTES of little-endian int16 PCM (wav_format "pcm"/"PCM"; anything else returns nullptr: the
// reference would hand it to ffmpeg).  Returns nullptr on a bad handle/format, a result with empty msg for empty audio.
FUNASR_RESULT FunOfflineInferBuffer(FUNASR_HANDLE handle, const char* sz_buf, int n_len, FUNASR_MODE mode,
                                    QM_CALLBACK fn_callback, const std::vector<std::vector<float>>& hw_emb,
                                    int sampling_rate = 16000, std::string wav_format = "pcm", bool itn = true,
                                    int vad_tail_sil = 800, int vad_max_len = 60000, FUNASR_DEC_HANDLE dec_handle = nullptr,
                                    std::string svs_lang = "auto", bool svs_itn = true);
const std::vector<std::vector<float>> CompileHotwordEmbedding(FUNASR_HANDLE handle, std::string& hotwords, ASR_TYPE mode = ASR_OFFLINE);
const char* FunASRGetResult(FUNASR_RESULT result, int n_index);
const char* FunASRGetStamp(FUNASR_RESULT result);
float FunASRGetRetSnippetTime(FUNASR_RESULT result);
void FunASRFreeResult(FUNASR_RESULT result);
void FunOfflineUninit(FUNASR_HANDLE handle);

// ---- 2-pass slice (funasrruntime.h:121-132; funasrruntime.cpp:52-63, 491-646, 816-842) ---------------------------------------
//   FunTpassInit         TpassStream: offline model (MODEL_DIR) + online model (ONLINE_MODEL_DIR) + VAD (VAD_DIR), shared
//   FunTpassOnlineInit   TpassOnlineStream: one per connection — ParaformerOnline stream, FsmnVadOnline, Audio
//   FunTpassInferBuffer  LoadPcmwavOnline -> Split (online VAD) -> streaming Forward per chunk -> offline Forward per closed
//                        segment; msg = text of this call's streaming chunks, tpass_msg = 2nd-pass text of a segment that
//                        closed in this call; with PUNC_DIR both go through punc_online_handle->AddPunc with punc_cache[0] /
//                        punc_cache[1] as in the reference (:543-556, :609-614) — the realtime class when the directory
//                        name contains "realtime" (tpass-stream.cpp:124-134)
FUNASR_HANDLE FunTpassInit(std::map<std::string, std::string>& model_path, int thread_num);
FUNASR_HANDLE FunTpassOnlineInit(FUNASR_HANDLE tpass_handle, std::vector<int> chunk_size = {5, 10, 5});
FUNASR_RESULT FunTpassInferBuffer(FUNASR_HANDLE handle, FUNASR_HANDLE online_handle, const char* sz_buf, int n_len,
                                  std::vector<std::vector<std::string>>& punc_cache, bool input_finished = true,
                                  int sampling_rate = 16000, std::string wav_format = "pcm", ASR_TYPE mode = ASR_TWO_PASS,
                                  const std::vector<std::vector<float>>& hw_emb = {{0.0f}}, bool itn = true, int vad_tail_sil = 800,
                                  int vad_max_len = 60000, FUNASR_DEC_HANDLE dec_handle = nullptr, std::string svs_lang = "auto",
                                  bool svs_itn = true);
const char* FunASRGetTpassResult(FUNASR_RESULT result, int n_index);
void FunTpassOnlineUninit(FUNASR_HANDLE online_handle);
void FunTpassUninit(FUNASR_HANDLE handle);

// Inspection for tests: token ids per VAD segment in time order and the segments (samples) of the last result.
const std::vector<std::vector<int>>& FunASRGetSegmentIds(FUNASR_RESULT result);
const std::vector<std::pair<int, int>>& FunASRGetSegments(FUNASR_RESULT result);
// ... the ids the streaming chunks of one FunTpassInferBuffer call emitted
const std::vector<int>& FunASRGetOnlineIds(FUNASR_RESULT result);
// Extensions without a counterpart in funasrruntime.h (the reference's GreedySearch keeps only the arg-max, paraformer.cpp:386-395):
// FunOfflineSetNbest(h, k), k = 1..8, makes every following FunOfflineInferBuffer on the handle ask the head for the k best
// candidates per token (ParaformerHip::SetNbest; 0 = off, the default: the adapter then calls exactly what it always called).
// FunASRGetTokenConfidence: exp(log-probability of the greedy token) for every token the text of the result was made from -- ids
// that Vector2StringV2 drops are dropped here too -- the VAD segments concatenated in time order as the text is; empty when the
// result was made without FunOfflineSetNbest.
void FunOfflineSetNbest(FUNASR_HANDLE handle, int k);
const std::vector<float>& FunASRGetTokenConfidence(FUNASR_RESULT result);
// The same for the 2-pass handle: FunTpassSetNbest(tpass_handle, k) applies SetNbest(k) to the second-pass model -- so that
// FunASRGetTokenConfidence covers the tpass text of a FunTpassInferBuffer result as it covers the offline text -- and
// ParaformerOnlineHip::SetDetail(k, true) to every stream made by a LATER FunTpassOnlineInit (0 = off, the default).
// FunASRGetOnlineConfidence / FunASRGetOnlineFireMs are parallel to FunASRGetOnlineIds (one entry per id, nothing dropped):
// exp(log-probability) of each streamed token and the time of the LFR row it fired in, in ms from the first sample the
// connection's stream saw since its last final chunk (fire frame * 60: the row's position to within the 25-ms analysis window and
// the 60-ms row).  Empty without FunTpassSetNbest.
void FunTpassSetNbest(FUNASR_HANDLE tpass_handle, int k);
const std::vector<float>& FunASRGetOnlineConfidence(FUNASR_RESULT result);
const std::vector<int>& FunASRGetOnlineFireMs(FUNASR_RESULT result);
// Time stamps from the CIF scan for any Paraformer (an extension: the reference stamps only through the CifPredictorV3 head of its
// 4-output graph, paraformer.cpp:545, and FunASRGetStamp is empty for every other model).  FunOfflineSetCifStamps(h, mode) applies
// ParaformerHip::SetCifTimestamps(mode) to the handle's acoustic model for every following FunOfflineInferBuffer: 0 = off (default:
// the adapter calls exactly what it always called), 1 = models without the head get stamps from the fire frames of the CIF scan, models
// with the head keep the head's, 2 = every model gets the CIF rule's (the head is skipped).  The result's stamps come through
// FunASRGetStamp in its usual "[[b,e],...]" form, one pair per character of the text, VAD segment offsets added; resolution is one
// LFR row (60 ms), and they are not the head's stamps.  FunTpassSetCifStamps does the same for the offline pass of the 2-pass flow.
void FunOfflineSetCifStamps(FUNASR_HANDLE handle, int mode);
// A token n-gram language model for the handle's acoustic model (an extension; ParaformerHip::InitTokenLm /
// SenseVoiceSmallHip::InitTokenLm): an ARPA file over the model's own tokens — not LM_DIR's TLG.fst, which is read (or not) as before.
// From then on an inference call with a FunASRCtcDecoderInit handle searches with the model, hotwords or none.  1: loaded, 0: not.
int FunOfflineLoadTokenLm(FUNASR_HANDLE handle, const char* arpa_path, float scale = 1.0f, float token_bonus = 0.0f);
int FunTpassLoadTokenLm(FUNASR_HANDLE tpass_handle, const char* arpa_path, float scale = 1.0f, float token_bonus = 0.0f);
// Time stamps for SenseVoiceSmall by CTC forced alignment (an extension: the reference's SenseVoiceSmall fills no stamps).
// FunOfflineSetCtcStamps(h, on) switches what SenseVoiceSmallHip::SetCtcTimestamps switches, for every following FunOfflineInferBuffer
// on the handle (nothing on a Paraformer handle); the switch is kept on the handle and applied call by call — the adapter's
// AlignGreedyTokens right behind each batch's Forward — so that a call which gets no stamps pays for no alignment.  Off (default) the
// adapter calls exactly what it always called; on, the tokens of the greedy text are aligned against the CTC rows (pfhip_svs_align) and
// FunASRGetStamp holds "[[b,e],...]" in ms, one pair per text token (the kept ids behind the four tags), VAD segment offsets added;
// resolution is one LFR row (60 ms).  A call with a decoder attached (dec_handle != nullptr) gets NO stamps and runs no alignment: a
// search returns a string, not the ids an alignment needs — except a CtcPrefixDecoderHip (FunASRCtcDecoderInit below), whose device
// search returns ids: the stamps are then those of its best hypothesis.  Forward and alignment are two calls: when more threads call the handle
// than it has execution contexts (PFHIP_INFLIGHT), another thread's forward can take the context in between; the alignment is then
// refused (never run against foreign rows) and THAT batch's segments come back without stamps — under such load FunASRGetStamp of a
// SenseVoice result may be empty or lack some segments' pairs.
void FunOfflineSetCtcStamps(FUNASR_HANDLE handle, int on);
// The per-connection decoder of a server without an LM (FunASRWfstDecoderInit's CtcPrefixDecoder branch, funasrruntime.cpp:836-894;
// FunWfstDecoderLoadHwsRes / UnloadHwsRes / FunASRWfstDecoderUninit): FunASRCtcDecoderInit makes a CtcPrefixDecoderHip
// (ctc_prefix_decoder_hip.h) on the vocabulary of the handle's SenseVoice model, or of its Paraformer; asr_type says
// whether `handle` is a FunOfflineInit or a FunTpassInit handle.  Passed as dec_handle to FunOfflineInferBuffer /
// FunTpassInferBuffer it selects the CTC prefix beam search ON THE DEVICE, with first beam (int)glob_beam, second beam
// (int)lat_beam (1..16 each) and the hotwords loaded into it; the text is the search's best hypothesis, and with
// FunOfflineSetCtcStamps / FunTpassSetCtcStamps on, FunASRGetStamp holds the spans of ITS tokens.  Any other dec_handle is, for a
// SenseVoice model, not passed on (as before).  FunCtcDecoderLoadHwsRes returns the hotwords that entered the graph (one with a
// piece outside the vocabulary is skipped); an empty map changes nothing.
// A Paraformer (offline, or the 2-pass second pass) is handed such a handle too — an extension: the reference creates the decoder
// and, without an LM, never looks at it (paraformer.cpp:563-579).  With hotwords loaded ParaformerHip runs
// pfhip_offline_forward_bias (width min((int)glob_beam, 8), beam min((int)lat_beam, 16), n best 1): text, FunASRGetSegmentIds, stamps
// and confidences are those of the search's best hypothesis, one token per row of the same forward.  With no hotword loaded, with an
// LM, or with any other dec_handle the call is exactly what it is without a handle.
FUNASR_DEC_HANDLE FunASRCtcDecoderInit(FUNASR_HANDLE handle, float glob_beam, float lat_beam, ASR_TYPE asr_type = ASR_OFFLINE);
int FunCtcDecoderLoadHwsRes(FUNASR_DEC_HANDLE dec_handle, int inc_bias, std::unordered_map<std::string, int>& hws_map);
void FunCtcDecoderUnloadHwsRes(FUNASR_DEC_HANDLE dec_handle);
void FunCtcDecoderUninit(FUNASR_DEC_HANDLE dec_handle);
void FunTpassSetCifStamps(FUNASR_HANDLE tpass_handle, int mode);
// The 2-pass sibling of FunOfflineSetCtcStamps, for a FunTpassInit handle whose MODEL_DIR names MODEL_SVS (the second pass is then a
// SenseVoiceSmallHip: FunTpassInferBuffer's trailing svs_lang / svs_itn go to its Forward, tpass_msg is its text with no punctuation
// and no ITN, funasrruntime.cpp:583-587, :609-631).  On: FunASRGetStamp of a result holds, per closed segment, "[[b,e],...]" — the
// spans of the greedy tokens (one LFR row = 60 ms) plus the segment's global start.  FunASRGetSegmentIds / FunASRGetSegments of such
// a result hold the second-pass ids and [start_ms, end_ms] of the segments closed in the call.
void FunTpassSetCtcStamps(FUNASR_HANDLE tpass_handle, int on);
// ... and the C-ABI handle of the offline acoustic model behind a FunOfflineInit handle (pfhip_inflight_stats in the harnesses)
struct pfhip_model;
pfhip_model* FunOfflineGetAsrHandle(FUNASR_HANDLE handle);
