// libravvent_hip.so -- host side of the C-ABI declared in include/ravvent_hip.h.
// Owns device memory, the stream, the decode hipGraph cache and the launch sequence that
// stands behind Basecaller.beam_search_prediction / greedy_search_prediction
// (/root/reference/basecaller.py:296-330).  No CPU compute path exists in this library.
#include "../../include/ravvent_hip.h"
#include "common.h"
#include "weight_images.h"
#include "signal_prep.h"
#include "stitch.h"

#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <tuple>
#include <vector>

// A stitch buffer (rv_stitch_open): device tables of n chunk rows that stitch slabs write and rv_stitch_run reads -- the calls' bases,
// probs [n, steps] and lengths [n], the four position values [n, steps] -- and on the host the window rows as the slabs stated them
struct RvStitchBuf {
  int n = 0, L = 0, steps = 0;
  uint8_t* bases = nullptr;
  float* probs = nullptr;
  int32_t* lens = nullptr;
  float* mv[4] = {nullptr, nullptr, nullptr, nullptr};      // raw_pos, raw_mass, event_pos, event_mass
  std::vector<int32_t> win;                                 // [n,5]; read_id -1: a row no slab has written
  int tickets = 0;                                          // uncollected tickets that write into it
};

namespace {

std::string g_create_error;

struct LstmW { const float *W, *U, *b; };

struct ProfEntry { double ms = 0; int64_t n = 0; };

constexpr int RV_MAX_ASYNC = 16;

struct GraphKey {
  int B, W, Tm, L, greedy, taps, split;
  bool operator<(const GraphKey& o) const {
    return std::tie(B, W, Tm, L, greedy, taps, split) < std::tie(o.B, o.W, o.Tm, o.L, o.greedy, o.taps, o.split);
  }
};

// whole-slab graphs: everything of a call that ends up in a frozen kernel argument or decides which kernels run
struct SlabKey {
  int B, T_r, T_e, W, L, flags;             // flags: greedy | calls << 1 | host inputs << 2 | host outputs << 3 | projecting layers >= 1 (Plan::fused_inproj) << 4
  uint64_t lut;                             // the fused post-processing's letter table travels by value in a kernel argument
  bool operator<(const SlabKey& o) const {
    return std::tie(B, T_r, T_e, W, L, flags, lut) < std::tie(o.B, o.T_r, o.T_e, o.W, o.L, o.flags, o.lut);
  }
};

// What rv_set_option sets, on the handle.  A slab context reads them through its handle while it queues a call (enqueue), never later
struct Options {
  int split = 1;                            // concurrent decode sub-slabs (1..4); measured neutral at B=256
  int att_nt = 0;
  int side_ev = 1;                          // event chain on a side stream under the raw in-projection GEMM
  int persist = 1;                          // whole beam-search loop in one launch, attention memory register-resident
  int flash = 1;                            // single-pass Luong attend (two-pass when 0 / Bahdanau)
  int split_proj = 2;                       // fused projection on split-bf16 MFMAs (six part products, f32-equivalent); 0 = f32 MFMAs
  int mx_att = 1;                           // persistent decode (Luong, one cell): attention on the matrix pipe
  int mx_cell = 1;                          // ... and its cell product [ctx' | h] . Wcat2 as well (needs mx_att)
  int wide = 1;                             // matrix-pipe recurrence, 16 chunks per workgroup: 1 on (default: every call runs the same kernels whatever its slab
                                            // size, so results do not depend on how a read is cut into slabs / shards), 0 packed-FMA kernels, -1 per-call choice
  int lane_inproj = 1;                      // the event encoder's layer-0 input projection inside its matrix-pipe recurrence (0: k_inproj_small + pre-projected inputs)
  int tail_wave = 1;                        // layer 0: cell update on a ninth wave, two row groups half a step apart
  int fuse = 1;                             // layers >= 1: input projection inside the recurrence kernel (MFMA waves)
  int fused_mem = 1;                        // option "fused_memory": the default decode form projects its own attention memory (no gemm_memory launch)
  int fused_inproj = -1;                    // option "fused_inproj": BiLSTM layers >= 1 of a sixteen-chunk matrix-pipe call project their own inputs
                                            // (k_lstm_rec_mx_proj: no k_gemm_ws launch, no xw round trip); 1 wherever the sixteen-chunk form runs, 0 never, -1 per call (fused_inproj_wanted)
  int taps = 0, graph = 1, profile = 0;
  int ptaps = 0;                            // persist_taps: per-step logits of the persistent decode (debug)
  int slab_graph = 0;                       // option "slab_graph": off by default -- measured (tools/graph_ab.py, C3, depth 10): a submit costs the host
                                            // 22-27 us instead of 43-48, but the replayed slabs stream 1.5-3 % SLOWER (354-361 k against 361-370 k chunks/s
                                            // settled; the runtime's per-node barrier packets), and the host is not what bounds the stream
  int gen = 0;                              // bumped by every rv_set_option / rv_load_weights: frozen arguments may have changed
  int async_depth = 2;                      // contexts the asynchronous entry points rotate through (1..RV_MAX_ASYNC)
  int coalesce = -1;                        // 0 / 1 off, n >= 2 slabs per group, -1 chosen from async_depth (coalesce_n)
  int group_inplace = 1;                    // a group's layer-0 kernels read its members' device inputs where they are (no copies into the group's buffers)
  int group_side_ev = -1;                   // a group's event encoder on a side stream beside its raw encoder: 0 / 1, -1 where the queues allow it (group_side_ev)
  int weight_parts = 2;                     // option "weight_parts": f16 parts a weight image keeps of each weight, as of the next rv_load_weights (round_blob_weights)
  int parts_loaded = 2;                     // ... and what the images in force were built with
  int one_part = 1;                         // option "one_part_kernels": weight_parts 1 decodes with k_dec_persist_1p where a form exists (0: the two-part kernels on the zero-lo images)
  int gru_persist = 0;                      // option "gru_persistent" (a GRU handle of one decoder cell): the one-launch persistent decode, k_dec_persist_gru, where a form serves the call
};

// Device images derived from the weights (weight_images.h lists them; rv_load_weights uploads what build_weight_images returns).  The
// handle owns them; every slab context reads them there
struct WeightImages {
#define X(T, name, count) T* name = nullptr;
  RV_WEIGHT_IMAGES(X)
#undef X
};
static_assert(wimg::U == RV_U && wimg::E == RV_E && wimg::MAX_VOCAB == RV_MAX_VOCAB, "weight_images.h restates common.h");
// ... and those of a GRU handle's persistent decode (wimg::GruPersistImages): allocated when option "gru_persistent" is first set to 1
struct GruPersistDev {
#define X(T, name, count) T* name = nullptr;
  RV_GRU_PERSIST_IMAGES(X)
#undef X
  bool allocated = false, built = false;    // built: they hold the images of the weights in force
  wimg::ImageScales scales;
};

// What a recording leaves behind for rv_get_tensor beside lB .. lptaps; a slab graph stores them at its capture and puts them back at every replay
struct SlabFacts {
  int lflash = 0, lkeys = 0, lpersist = 0, lsplit = 1, lW = 0;
  int lmem2_stale = 0;                      // the last call's decode projected its own memory without persist_taps: mem2 is built when "projected_memory" is asked for
};

struct CallsOut { const uint8_t* lut; uint8_t* bases; int32_t* lengths; float* probs; };

// The labels and score outputs of a forced decode (rv_teacher_forced*) or of rv_score_logits
struct ForcedCall { const int32_t* targets; uint32_t omit_mask; const RvScore* out; };

// One call as its entry point states it.  dev_out: tokens / out2 are device pointers written by the finalize kernel; else the results
// wait in pinned memory for finish().  lut != nullptr: the fused post-processing (rv_beam_search_calls) instead of tokens / scores.
struct Call {
  const float *raw = nullptr, *ev = nullptr;
  bool dev_in = false;
  int B = 0, T_r = 0, T_e = 0, W = 1, L = 0;
  bool greedy = false;
  int32_t* tokens = nullptr;
  float* out2 = nullptr;
  bool dev_out = false;
  const uint8_t* lut = nullptr;             // the letter table of the fused post-processing
  const CallsOut* calls = nullptr;          // ... and its host outputs (synchronous calls; an asynchronous one names them at its collect)
  bool whole_beam = false;                  // rv_beam_search_all* / rv_beam_search_submit_all*: every beam, through ...
  const RvBeams* beams = nullptr;           // ... these outputs (null: an asynchronous call with host outputs, named at its collect)
  const ForcedCall* forced = nullptr;       // rv_teacher_forced*
  bool want_moves = false;                  // rv_beam_search_moves* / rv_beam_search_submit_moves (always with whole_beam): the moves too, through ...
  const RvMoves* moves = nullptr;           // ... these outputs (null: an asynchronous call, named at its collect)
  bool want_call_moves = false;             // rv_beam_search_*calls_moves (always with lut): a position per called letter, through ...
  const RvCallMoves* call_moves = nullptr;  // ... these host outputs (null: an asynchronous call, named at its collect)
  const RvMoves* forced_moves = nullptr;    // rv_teacher_forced_moves* (always with forced): the moves of the forced decode, [B,L-1]
  // rv_beam_search_windows*: the chunks are windows of reads on the device (raw / ev unset, dev_in set).  As the entry point states it: its
  // table's rows, resolved and checked against their reads (resolve_windows), in host memory; past enqueue()'s staging: the context's device
  // copy of them.  win_expand (set by enqueue): the call takes a path whose layer-0 kernels read chunk tensors, so k_expand_windows writes
  // them into the context's input buffers first and raw / ev name those
  const RecWindow* windows = nullptr;
  bool win_expand = false;
  // rv_beam_search_submit_windows_stitch (always with want_call_moves): the slab's results go device-to-device into rows stitch_row0 .. of
  // this buffer on the slab's stream instead of into the staging of a host caller
  RvStitchBuf* stitch = nullptr;
  int stitch_row0 = 0;
};

// A read on the device (rv_read_put*): its scaled samples [n_raw] and scaled events [n_ev,5].  owned: the buffers are the handle's (a
// dropped read keeps them for the next put that fits); else the caller's (rv_read_put_dev).  users: uncollected tickets whose tables name it
struct Read {
  float *d_raw = nullptr, *d_ev = nullptr;
  size_t n_raw = 0, n_ev = 0, cap_raw = 0, cap_ev = 0;      // cap_*: floats the owned buffers hold
  float* pin = nullptr; size_t pin_cap = 0;                 // pinned staging of the upload: the caller's buffers are free when the put returns
  bool live = false, owned = false, used = false;
  int users = 0, id = -1;
  // a read made from its signal (rv_read_put_signals) also keeps its event arrays [n_ev] and its window table [n_win,4] for rv_read_fetch
  bool prepped = false;
  int64_t *d_est = nullptr, *d_eln = nullptr;
  double *d_emu = nullptr, *d_esd = nullptr;
  int32_t* d_win = nullptr;
  size_t cap_evd = 0, cap_win = 0, n_win = 0;               // cap_evd: events the four arrays hold; cap_win: window rows
  // the event starts and lengths [n_xev] a caller gave for a read put by rv_read_put / _dev (rv_read_put_events), for the stitch; they
  // belong to the read whose id is ev_id (a slot taken again keeps the buffers, not the table)
  int64_t *d_xst = nullptr, *d_xln = nullptr;
  size_t cap_xev = 0, n_xev = 0;
  int ev_id = -2;
};

// The handle's scratch of a stitch (rv_stitch_calls, rv_stitch_run), reused and grown: per chunk, per read, per base of the outputs
struct StitchScratch {
  StChunk* chunks = nullptr; size_t cap_chunks = 0;
  int2* keep = nullptr; size_t cap_keep = 0;
  long long* off = nullptr; size_t cap_off = 0;
  long long* tiles = nullptr; size_t cap_tiles = 0;
  StRead* reads = nullptr; size_t cap_reads = 0;
  int32_t* rows = nullptr; size_t cap_rows = 0;
  long long *read_off = nullptr, *pin_read_off = nullptr; size_t cap_read_off = 0, cap_pin = 0;
  uint8_t* o_bases = nullptr; size_t cap_o_bases = 0;
  float* o_f[3] = {nullptr, nullptr, nullptr}; size_t cap_o_f[3] = {0, 0, 0};      // probs, raw_mass, event_mass
  double* o_pos = nullptr; size_t cap_o_pos = 0;
  int32_t* o_i[2] = {nullptr, nullptr}; size_t cap_o_i[2] = {0, 0};              // source_chunk, source_index
  // the tables of rv_stitch_calls, which brings them from the host (rv_stitch_run reads those of its stitch buffer)
  uint8_t* in_bases = nullptr; size_t cap_in_bases = 0;
  float* in_f[5] = {nullptr, nullptr, nullptr, nullptr, nullptr}; size_t cap_in_f[5] = {0, 0, 0, 0, 0};      // probs and the four position values
  int32_t* in_len = nullptr; size_t cap_in_len = 0;
};

// The handle's scratch of rv_read_put_signals, reused from batch to batch: per sample (cap_x), per tile (cap_tiles), per read (cap_reads)
struct SignalScratch {
  int16_t *d_x = nullptr, *pin_x = nullptr;
  double *ps = nullptr, *pq = nullptr, *t1 = nullptr, *t2 = nullptr;
  uint2* bounds = nullptr;
  long long* tile_sums = nullptr;
  double* var_part = nullptr;
  SpRead *d_reads = nullptr, *pin_reads = nullptr;
  int *d_cnt = nullptr, *pin_cnt = nullptr;                 // [2][cap_reads]: events, windows
  double* fit = nullptr;
  size_t cap_x = 0, cap_tiles = 0, cap_reads = 0;
};

// What a recording needs beyond the call, resolved once before enqueue() (begin_all_beams, begin_forced, launch_group)
struct CallParts {
  bool whole_beam = false;                  // k_dec_finalize_beams in k_dec_finalize's place, writing to ...
  BeamsOut beams{};                         // ... these device addresses (the caller's, or the context's d_beams)
  bool moves = false;                       // the decode leaves step_moves records and k_dec_finalize_moves runs behind k_dec_finalize_beams, writing to ...
  MovesOut moves_out{};                     // ... these device addresses (the caller's, or the context's d_moves)
  bool call_moves = false;                  // a calls slab whose decode leaves the records too: k_dec_finalize_calls_moves runs behind k_dec_finalize, ...
  bool forced_moves = false;                // ... a forced decode's: k_forced_moves does; either writes through moves_out, [B,L-1]
  bool records() const { return moves || call_moves || forced_moves; }      // the decode leaves step_moves records
  const int* labels = nullptr;              // a forced decode feeds these label rows [B,L] (device: the caller's, or d_forced) instead of its argmax
  ScoreArgs score{};                        // ... and scores them: omit_mask and the output addresses (device: the caller's, or the d_sc_* buffers; null = not asked for)
  const DecMembers* members = nullptr;      // the member table of a group's internal call
  int form_B = -1;                          // the B that picks the kernel forms (a group: its first member's), -1 = the call's own
};

// Which kernels a call runs: decided once, before anything is queued (plan_call), and carried by the recording (Slab)
struct Plan {
  bool wide = false;                        // encoder recurrences on the matrix pipe (lstm_mx.hip; a GRU handle: always) ...
  bool rows8 = false;                       // ... with eight chunks per workgroup (the latency form)
  bool fused_inproj = false;                // ... with layers >= 1 projecting their own inputs (sixteen chunks only: k_lstm_rec_mx_proj)
  int persist = -1;                         // the form of the one-launch persistent decode (dec_persist_form), or -1: the per-step kernels
  bool flash = false;                       // single-pass Luong attend (wider beams: register budget -> two-pass)
  bool keys = false;                        // the key GEMM runs: the two-pass attend, the "keys" debug tap, a moves call on the per-step kernels
  bool win_lane = false;                    // a window call gathers its chunks in the lane of the layer-0 recurrence (else behind k_expand_windows)
  bool graphable = false;                   // the call replays as a slab graph (option "slab_graph")
};

struct SlabCtx;
struct Group;

// One uncollected slab of a coalesced group; `done`: its group has run, S is final
struct Tick { bool busy = false, done = false, dev_out = false, calls = false; int ticket = -1, member = 0, B = 0, row0 = 0, steps = 0, S = 0; Group* grp = nullptr; };

}  // namespace

// The handle a caller holds: the weights and what is derived from them, the options, the slab contexts and groups its calls run on,
// the tickets and the reads.  Nothing of a call in flight lives here (SlabCtx, Group)
struct RvContext {
  RvConfig cfg{};
  int rnn = RV_RNN_BILSTM;                  // cell family (rv_create_rnn)
  std::string err;
  std::vector<void*> allocs;                // the blob and the images

  // weights
  float* d_w = nullptr;
  size_t n_w = 0;
  bool loaded = false;
  std::vector<std::vector<LstmW>> enc[2];   // [enc][layer][dir]
  std::vector<LstmW> dec;                   // stacked decoder cells
  WeightImages img;                         // derived from the weights
  const float *W_mem = nullptr, *W_q = nullptr, *v_att = nullptr, *W_att = nullptr, *W_fc = nullptr, *b_fc = nullptr;
  wimg::ImageScales scales;                 // the weight-derived scalars of the decode (set by rv_load_weights)
  GruPersistDev gimg;                       // a GRU handle under option "gru_persistent"

  Options opt;
  int dbg_role = 0;                         // timing probe (RV_DBG_ROLE): 1 = no projection math, 2 = no recurrence math
  std::map<std::string, ProfEntry> prof;

  // Slab contexts by slot -- own stream, own buffers -- so that several slabs are in flight on the GPU at once.  Slot 0 exists from
  // rv_create_rnn on and serves the synchronous calls, the debug taps and rv_get_tensor; the asynchronous calls (rv_beam_search_submit* /
  // rv_beam_search_collect*) rotate through slots 0 .. async_depth - 1, created on the first submit that needs them
  std::vector<SlabCtx*> slabs;
  int inflight_hint = 1;                    // slabs the caller keeps in flight (1 for the synchronous entry points): sizes the workgroups
  int next_slot = 0, generation = 0;
  int lS = 0;                               // S of the last call rv_get_tensor answers for (DESIGN.md section 16 has the one quirk)

  // coalesced asynchronous calls (option "coalesce"): up to n consecutively submitted slabs of the default streamed path are decoded as ONE
  // internal call of sum(B) chunks on a group's context, whose buffers hold n x max_batch chunks -- so that the narrow recurrence launches
  // are n times as wide and a handle fills the chip from few hardware queues.  Tickets stay per slab (`ticks`).
  std::vector<Group*> groups;               // created when a slab finds none idle
  Group* open_grp = nullptr;                // the group that still takes members: filled, not launched
  Tick ticks[RV_MAX_ASYNC];
  long long co_groups = 0, co_slabs = 0, co_largest = 0;     // "coalesce_stats": groups launched, slabs in them, members of the largest
  FormLog gforms;                           // the instantiations the last coalesced group launched on its own context ("group_kernel_forms")

  // window calls (rv_beam_search_windows*): the reads, the stream and event of their uploads, and which reads each uncollected ticket uses
  std::vector<Read> reads;
  hipStream_t copy_stream = nullptr;
  hipEvent_t ev_put = nullptr;              // recorded behind every upload: a window call's stream waits for it, the host never does
  long long read_allocs = 0, read_puts = 0; // "read_stats": device allocations made for reads, puts
  long long win_expands = 0;                // ... and launches of k_expand_windows
  int read_gen = 0;
  std::map<int, std::vector<int>> ticket_reads;
  SignalScratch sp;                         // rv_read_put_signals
  // stitching by signal position (rv_stitch_*): the buffers that are open, which uncollected ticket writes into which, the scratch
  std::vector<RvStitchBuf*> stitch_bufs;
  std::map<int, RvStitchBuf*> stitch_tickets;
  StitchScratch st;
};

namespace {

// What one slab in flight needs: a stream, the per-slab buffers, the decode state and graphs, the last call's facts and one pending
// call.  Options, weights, images and scales are its handle's
struct SlabCtx {
  RvContext* h = nullptr;
  int slot = 0;                             // its place in h->slabs (-1: a group's context)
  Group* grp = nullptr;                     // the group it belongs to (null: a plain slab context)
  int cap = 0;                              // chunks its buffers hold: the handle's max_batch (a group's context: times its members)
  hipStream_t stream = nullptr;
  std::vector<void*> allocs;
  hipStream_t side[3] = {nullptr, nullptr, nullptr};
  hipEvent_t ev_fork = nullptr, ev_join[3] = {nullptr, nullptr, nullptr};

  // Debug taps and rv_get_tensor belong to slot 0: every other context runs with both tap options off, whatever the handle says
  bool own() const { return slot == 0; }
  int taps() const { return own() ? h->opt.taps : 0; }
  int ptaps() const { return own() ? h->opt.ptaps : 0; }

  int* d_chunk_steps = nullptr;
  float* mem2 = nullptr;                    // [B,Tm,256] = enc_out . Wmp: keys | attention-layer image of the values
  // encoder buffers
  float *d_raw = nullptr, *d_ev = nullptr;
  uint8_t* mask = nullptr;
  float* act[2][2] = {{nullptr, nullptr}, {nullptr, nullptr}};   // [enc][pingpong]
  float* xw[2] = {nullptr, nullptr};   // per encoder (the two encoders run on concurrent streams)
  float* st[2][2][4] = {};             // [enc][set][h_f, c_f, h_b, c_b]
  float *enc_out = nullptr, *keys = nullptr;
  // decoder buffers
  DecState dec_st{};
  float* step_align = nullptr; size_t step_align_cap = 0;
  float* palign = nullptr; size_t palign_cap = 0;   // persist_taps: alignments of the persistent decode
  int32_t* out_tokens = nullptr;
  float* out2 = nullptr;
  // pinned host staging for the host-buffer entry points (pageable hipMemcpy is synchronous and slow)
  float *pin_raw = nullptr, *pin_ev = nullptr, *pin_out2 = nullptr;
  int32_t* pin_tok = nullptr;
  int* pin_S = nullptr;
  uint8_t *d_bases = nullptr, *pin_bases = nullptr;
  float *d_probs = nullptr, *pin_probs = nullptr;
  int *d_clen = nullptr, *pin_clen = nullptr;
  // the whole beam (rv_beam_search_all*): device outputs and pinned staging of the host variants, [cap, max_output_len, max_beam]
  // and [cap, max_beam], allocated on this context's first such call (ensure_beam_buffers)
  BeamsOut d_beams{}, pin_beams{};
  // moves (rv_beam_search_moves*): the decode's records [max_output_len - 1, cap, max_beam, RV_MOVE_COLS], allocated on this context's
  // first such call (ensure_moves_buffers), and for the host variants the six outputs [cap, max_output_len, max_beam] with their staging
  float* d_step_moves = nullptr;
  MovesOut d_moves{}, pin_moves{};
  // forced decode and scoring (rv_teacher_forced*, rv_score_logits)
  int32_t* d_forced = nullptr;              // host variants: labels [cap, max_output_len] and the score outputs, allocated on this context's
  float *d_sc_nll = nullptr, *d_sc_sum = nullptr;   //   first such call (ensure_score_buffers): nll [cap, max_output_len], nll_sum [cap],
  int32_t* d_sc_cnt = nullptr;              //   n_labels | n_match | n_counted [3][cap]

  long long* rec_ts = nullptr;              // diagnostic: per-wave cycle sums of the raw layer-0 recurrence (RV_REC_STAMPS=1) or of its fused layer 1 (=2)
  int rec_ts_layer = 0;
  struct Pending { std::string name; hipEvent_t a, b; };
  std::vector<Pending> pending;             // profile events in flight: drained into the handle's profile when the call is finished
  std::vector<hipEvent_t> ev_pool;
  std::map<GraphKey, hipGraphExec_t> graphs;
  // one hipGraph per slab context and call shape: the whole slab (ten launches on the default path) replays as ONE hipGraphLaunch.
  // Every kernel argument is frozen at capture; the addresses that change from call to call (caller inputs and outputs) reach the
  // kernels through a 4-entry table in mapped pinned memory (common.h: RV_PTAB_*), rewritten by the host before each replay
  struct SlabGraph { hipGraphExec_t exec = nullptr; SlabFacts fact; };
  std::map<SlabKey, SlabGraph> slab_graphs;
  const void** d_ptab = nullptr;
  const void** pin_ptab = nullptr;
  int graph_gen = 0;                        // the handle's opt.gen this context's slab graphs were captured under

  // last call
  int lB = 0, lTm = 0, lL = 0, lgreedy = 0, ltaps = 0, lptaps = 0;
  int lmoves = 0;                           // it was a moves call: "step_moves" holds its records
  SlabFacts fact;
  FormLog lforms;                           // the kernel instantiations it launched ("kernel_forms"); lforms_ok = 0: it ran as a slab graph
  int lforms_ok = 1;
  std::map<GraphKey, FormLog> graph_forms;  // ... those a captured decode graph of `graphs` launches (recorded at its capture)
  struct PendingCall { bool busy = false, trivial = false, greedy = false, dev_out = false, calls = false, all = false, moves = false, cmoves = false, stitch = false; int B = 0, steps = 0, V = 0, Wd = 0, ticket = -1; } pend;

  // window calls (rv_beam_search_windows*): the resolved table of the call this context runs, [cap] rows -- written by the host into
  // pinned staging when the call is queued (a group: as its members come), copied to the device in front of the call's first kernel
  RecWindow *pin_win = nullptr, *d_win = nullptr;
};

// A group of coalesced slabs: the context its internal call runs on, and what its members add up to
struct Group {
  SlabCtx* ctx = nullptr;
  int cap = 0, n = 0, rows = 0, staged = 0, failed = RV_OK;     // members it takes / holds, chunks they add up to, members whose results wait in its staging
  bool launched = false, synced = false, dev_in = false, dev_out = false, calls = false;
  int Tr = 0, Te = 0, W = 0, L = 0;
  int B0 = 0;                               // its first member's B: the group takes the kernel forms that member would have got alone
  uint8_t lut[RV_MAX_VOCAB] = {};
  int tslot[RV_MAX_MEMBERS] = {};
  DecMembers members{};                     // its member table: output addresses as the members come (submit_group), rows at its launch (launch_group)
  bool inplace = false;                     // its members' device inputs are read in place (option "group_inplace"), through ...
  RecMembers in[2]{};                       // ... these tables [raw, event]: addresses as the members come, rows at its launch
  bool win = false;                         // its members are window slabs: their rows stand back to back in pin_win (a window slab and a chunk-tensor slab never share a group)
};

int fail(RvContext* h, int code, const char* fmt, ...) {
  char buf[512];
  va_list ap; va_start(ap, fmt); vsnprintf(buf, sizeof buf, fmt, ap); va_end(ap);
  if (h) h->err = buf; else g_create_error = buf;
  return code;
}

#define HIPCHK(h, expr)                                                                   \
  do {                                                                                    \
    hipError_t e_ = (expr);                                                               \
    if (e_ != hipSuccess)                                                                 \
      return fail(h, RV_EHIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
  } while (0)

#define TRY(x) do { int r_ = (x); if (r_ != RV_OK) return r_; } while (0)
// rv_create and the context's buffers: the short form of HIPCHK's message
#define HIPTRY(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) return fail(h, RV_EHIP, "%s: %s", #x, hipGetErrorString(e_)); } while (0)

int async_depth(const RvContext* h) { return std::min(std::max(h->opt.async_depth, 1), RV_MAX_ASYNC); }

// The next ticket of handle h for `slot` (a slab context, or an entry of `ticks`)
int issue_ticket(RvContext* h, int slot) {
  h->generation = (h->generation + 1) & 0xFFFFF;
  return (h->generation << 4) | slot;
}

// Device memory owned by the handle or by one of its slab contexts; a failure is the handle's
template <class T>
int dalloc(RvContext* h, std::vector<void*>& owned, T** p, size_t count) {
  void* q = nullptr;
  hipError_t e = hipMalloc(&q, std::max<size_t>(count, 1) * sizeof(T));
  if (e != hipSuccess) return fail(h, RV_ENOMEM, "hipMalloc(%zu bytes) failed: %s", count * sizeof(T), hipGetErrorString(e));
  owned.push_back(q);
  *p = static_cast<T*>(q);
  return RV_OK;
}
template <class T> int dalloc(RvContext* h, T** p, size_t count) { return dalloc(h, h->allocs, p, count); }
template <class T> int dalloc(SlabCtx* cx, T** p, size_t count) { return dalloc(cx->h, cx->allocs, p, count); }

void bind_weights(RvContext* h) {
  const wimg::BlobLayout lay(h->cfg, h->rnn);
  auto dev = [&](const wimg::CellOffsets& o) { return LstmW{h->d_w + o.W, h->d_w + o.U, h->d_w + o.b}; };
  for (int e = 0; e < 2; ++e) {
    h->enc[e].assign(h->cfg.enc_depth, std::vector<LstmW>(2));
    for (int l = 0; l < h->cfg.enc_depth; ++l)
      for (int dr = 0; dr < 2; ++dr) h->enc[e][l][dr] = dev(lay.cell(e, l, dr));
  }
  h->dec.clear();
  for (const wimg::CellOffsets& o : lay.dec) h->dec.push_back(dev(o));
  h->W_mem = h->d_w + lay.W_mem; h->W_q = h->d_w + lay.W_q; h->v_att = h->d_w + lay.v_att;
  h->W_att = h->d_w + lay.W_att; h->W_fc = h->d_w + lay.W_fc; h->b_fc = h->d_w + lay.b_fc;
}

// ---- profiling: bracket a launch with events on the launch stream
struct Scope {
  SlabCtx* cx; const char* name; hipEvent_t a = nullptr, b = nullptr; bool on; hipStream_t st;
  // profile 3: only the decode launches (the dominant kernel) are bracketed, so that the timed region of bench.py
  // carries two events per slab instead of two per launch (the per-launch events cost 2.6 % of a C3 slab)
  Scope(SlabCtx* x_, const char* n, hipStream_t st_ = nullptr, bool decode = false)
      : cx(x_), name(n), on(x_->h->opt.profile != 0 && (x_->h->opt.profile != 3 || decode)), st(st_ ? st_ : x_->stream) {
    if (!on) return;
    auto get = [&]() {
      hipEvent_t e;
      if (!cx->ev_pool.empty()) { e = cx->ev_pool.back(); cx->ev_pool.pop_back(); }
      else hipEventCreate(&e);
      return e;
    };
    a = get(); b = get();
    hipEventRecord(a, st);
  }
  ~Scope() {
    if (!on) return;
    hipEventRecord(b, st);
    cx->pending.push_back({name, a, b});
  }
};

void drain_profile(SlabCtx* cx) {
  for (auto& p : cx->pending) {
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, p.a, p.b) == hipSuccess) {
      ProfEntry& e = cx->h->prof[p.name];
      e.ms += ms; e.n += 1;
    }
    cx->ev_pool.push_back(p.a); cx->ev_pool.push_back(p.b);
  }
  cx->pending.clear();
}

// Side stream g of a context, created on first use.  Highest priority: their few workgroups should take CU slots as soon as they free up.
hipStream_t side_stream(SlabCtx* cx, int g) {
  if (!cx->side[g]) {
    int lo = 0, hi = 0;
    (void)hipDeviceGetStreamPriorityRange(&lo, &hi);
    if (hipStreamCreateWithPriority(&cx->side[g], hipStreamNonBlocking, hi) != hipSuccess) { cx->side[g] = nullptr; return cx->stream; }   // (degrades to in-order)
  }
  return cx->side[g];
}

int pick_rows_per_block(int B) {
  // one direction of BT chunks per workgroup, 2 directions: aim at <= 256 workgroups (1 per CU)
  int bt = (2 * B + 255) / 256;
  int r = 1;
  while (r < bt && r < 8) r <<= 1;
  return r;
}

// Encoder.call for one encoder (basecaller.py:48-59) writing into enc_out at time offset t_off.
// Does this slab run its encoder recurrences on the matrix pipe (lstm_mx.hip: 16 chunks of one direction per workgroup)?
bool wide_recurrence(const RvContext* h, int B, int T_r) {
  if (h->opt.wide == 0 || !h->opt.fuse) return false;
  if (h->cfg.mode != RV_MODE_EVENT && !lstm_rec_mx_window_fits(T_r)) return false;
  if (h->opt.wide > 0) return true;
  // Per-call choice (-1).  The packed-FMA kernels cost per chunk, the matrix forms per workgroup.  Synchronous calls at T = 300 + 30
  // (tools/rows8_ab.py, k chunks/s; FMA / matrix pipe with 8 / with 16 chunks per workgroup): 64 chunks 75 / 64 / 53; 128: 146 / 124 / 102;
  // 192: 159 / 181 / 150; 256: 203 / 224 / 189; 512: 208 / 298 / 266; 1,024: 212 / 342 / 341 -- FMA below 160 chunks in flight, the
  // eight-chunk form up to 512, sixteen above (less CU-time per chunk: what a stream of slabs wants).
  return (long long)B * std::max(h->inflight_hint, 1) >= 160;
}

// ... and with eight chunks per workgroup (two MFMAs per tile and k-step, half the cell update per lane: a shorter step on twice the
// workgroups)?  wide_recurrence = 2 always; = -1 (per-call choice) when the slabs in flight leave the chip room for it.
bool rows8_wanted(const RvContext* h, int B) {
  if (h->opt.wide == 2) return true;
  const long long n = (long long)B * std::max(h->inflight_hint, 1);
  return h->opt.wide < 0 && n >= 160 && n <= 512;
}

// Do layers >= 1 of a sixteen-chunk matrix-pipe call project their own inputs (k_lstm_rec_mx_proj) instead of reading xw from the split
// GEMM?  Both forms give the same bits, so the choice is free per call.  fused_inproj = 1 always; = -1 by the chunks in flight: one
// isolated slab is a latency chain, where the GEMM (0.12 ms at C3) plus the streaming layer beats the fused layer's longer steps; a
// stream of slabs is bound by CU-time, where the fused layer takes less of it (profiles/fused_inproj.md has the sweep).
constexpr long long FUSED_INPROJ_MIN_CHUNKS = 1280;
bool fused_inproj_wanted(const RvContext* h, int B) {
  if (h->opt.fused_inproj >= 0) return h->opt.fused_inproj == 1;
  return (long long)B * std::max(h->inflight_hint, 1) >= FUSED_INPROJ_MIN_CHUNKS;
}

// Does layer 0 of this encoder take x . W + b in the lane of its matrix-pipe recurrence, from LDS windows of the chunks' inputs?
bool lane_layer0(const RvContext* h, int F, int T) {
  return F == 1 || (F == 5 && h->opt.lane_inproj && lstm_rec_mx_window_fits(T, 5));
}

// Encoder.call of a GRU handle: k_gru_rec_mx on every layer.  Layer 0 takes x . W + b[0] in the lane and leaves the input mask; layers
// >= 1 read xw [B,T,2,384] from the split-f16 GEMM over three column blocks (both directions and their input biases in one launch).
// State sets hold h only: layer l + 1 starts from layer l's two final states.
void run_gru_encoder(SlabCtx* cx, int e, const float* x, int F, int B, int T, int Tm, int t_off, hipStream_t s, int l_begin, int l_end) {
  RvContext* const h = cx->h;
  const int depth = h->cfg.enc_depth;
  for (int l = std::max(l_begin, 0); l < std::min(depth, l_end); ++l) {
    const bool last = l == depth - 1;
    GruRecArgs a{};
    a.B = B; a.T = T;
    a.out = last ? cx->enc_out : cx->act[e][l & 1]; a.out_T = last ? Tm : T; a.out_t0 = last ? t_off : 0;
    const int rd = (l & 1) ^ 1, wr = l & 1;     // state sets: layer l reads set rd, writes set wr
    for (int dr = 0; dr < 2; ++dr) {
      const LstmW& w = h->enc[e][l][dr];
      a.W[dr] = w.W; a.b[dr] = w.b;
      a.Ua[dr] = h->img.gUa + ((size_t)(e * depth + l) * 2 + dr) * RV_GRU_UA_SLOT;
      a.h0[dr] = l > 0 ? cx->st[e][rd][2 * dr] : nullptr;
      a.hT[dr] = cx->st[e][wr][2 * dr];
    }
    if (l == 0) {
      a.x = x;
      a.mask = cx->mask; a.mask_T = Tm; a.mask_t0 = t_off; a.pad = h->cfg.padding_value;
      Scope sc(cx, F == 1 ? "gru_rec_raw_l0" : "gru_rec_event_l0", s);
      launch_gru_rec_mx(a, F, s, &cx->lforms);
      continue;
    }
    {
      const size_t slot = (size_t)(e * (depth - 1) + (l - 1));
      Scope sc(cx, e == 0 ? "gemm_inproj_raw" : "gemm_inproj_event", s);
      launch_gemm_split_blocks(cx->act[e][(l - 1) & 1], B * T, h->img.gWx16 + slot * RV_GRU_WX16_SLOT, 3, h->img.gbx + slot * 2 * RV_GG, cx->xw[e],
                               2 * RV_GG, s);
    }
    a.x = cx->xw[e];
    Scope sc(cx, e == 0 ? "gru_rec_raw_l1p" : "gru_rec_event_l1p", s);
    launch_gru_rec_mx(a, 0, s, &cx->lforms);
  }
}

void run_encoder(SlabCtx* cx, const Plan& plan, int e, const float* x, int F, int B, int T, int Tm, int t_off, hipStream_t s,
                 int l_begin = 0, int l_end = 1 << 30, const void* const* ptab = nullptr, const RecWindow* windows = nullptr) {
  RvContext* const h = cx->h;
  if (h->rnn == RV_RNN_BIGRU) return run_gru_encoder(cx, e, x, F, B, T, Tm, t_off, s, l_begin, l_end);      // (never with ptab or windows: enqueue)
  const int depth = h->cfg.enc_depth;
  const int bt = pick_rows_per_block(B);
  for (int l = std::max(l_begin, 0); l < std::min(depth, l_end); ++l) {
    const bool last = l == depth - 1;
    float* out = last ? cx->enc_out : cx->act[e][l & 1];
    RecArgs a{};
    a.B = B; a.T = T;
    a.out = out; a.out_T = last ? Tm : T; a.out_t0 = last ? t_off : 0;
    const int rd = (l & 1) ^ 1, wr = l & 1;     // state sets: layer l reads set rd, writes set wr
    for (int dr = 0; dr < 2; ++dr) {
      const LstmW& w = h->enc[e][l][dr];
      a.U[dr] = w.U;
      a.Up[dr] = h->img.Up + ((size_t)(e * depth + l) * 2 + dr) * RV_U * RV_G;
      a.Ua[dr] = h->img.Ua + ((size_t)(e * depth + l) * 2 + dr) * RV_UA_SLOT;
      a.h0[dr] = l > 0 ? cx->st[e][rd][2 * dr] : nullptr;
      a.c0[dr] = l > 0 ? cx->st[e][rd][2 * dr + 1] : nullptr;
      a.hT[dr] = cx->st[e][wr][2 * dr];
      a.cT[dr] = cx->st[e][wr][2 * dr + 1];
    }
    if (plan.wide) {
      // matrix-pipe recurrence.  Raw layer 0 folds its one-feature input projection in; every other layer reads pre-projected
      // inputs xw [B,T,2,512]: event layer 0 from a small elementwise kernel, layers >= 1 from the split-f16 GEMM (both directions
      // and their biases in one launch, A read once).
      if (l == 0 && lane_layer0(h, F, T)) {
        // layer 0 takes x . W + b in the lane, from LDS windows of its chunks' inputs: no projection launch, no xw round trip (round 4: the
        // event encoder's five features too -- the same fused multiply-adds in the same order as k_inproj_small: identical bits)
        a.x = x;
        for (int dr = 0; dr < 2; ++dr) { a.W[dr] = h->enc[e][0][dr].W; a.bias[dr] = h->enc[e][0][dr].b; }
        a.mask = cx->mask; a.mask_T = Tm; a.mask_t0 = t_off; a.pad = h->cfg.padding_value;   // the layer-0 kernels leave the input mask too
        a.ptab = ptab;
        if (cx->grp && cx->grp->inplace) a.members = cx->grp->in[e];    // (a group whose members' inputs stay where they are: launch_group)
        a.windows = windows;                           // (a window call on the default path: the chunks are gathered from their reads in the lane)
        a.dbg_ts = (e == 0 && cx->rec_ts_layer == 0) ? cx->rec_ts : nullptr;     // (RV_REC_STAMPS=1: phase cycle sums of workgroup (0, 0))
        Scope sc(cx, F == 1 ? "lstm_rec_raw_l0" : "lstm_rec_event_l0", s);
        launch_lstm_rec_mx(a, F, s, plan.rows8, &cx->lforms);
        a.dbg_ts = nullptr; a.ptab = nullptr; a.mask = nullptr; a.members.n = 0; a.windows = nullptr;
        continue;
      }
      if (l > 0 && plan.fused_inproj) {
        // the layer projects its own inputs from the previous layer's output: no projection launch, xw[e] untouched
        const size_t slot = (size_t)(e * (depth - 1) + (l - 1));
        a.x = cx->act[e][(l - 1) & 1];
        a.Wh[0] = h->img.Wx16 + slot * RV_WX16_SLOT;
        a.bias[0] = h->img.bx2 + slot * 2 * RV_G;
        Scope sc(cx, e == 0 ? "lstm_rec_raw_l1p" : "lstm_rec_event_l1p", s);
        launch_lstm_rec_mx_proj(a, s, &cx->lforms);
        continue;
      }
      if (l == 0) {
        Scope sc(cx, e == 0 ? "inproj_raw_l0" : "inproj_event_l0", s);
        launch_inproj_small(x, B * T, F, h->enc[e][0][0].W, h->enc[e][0][0].b, h->enc[e][0][1].W, h->enc[e][0][1].b, cx->xw[e],
                            cx->mask, T, Tm, t_off, h->cfg.padding_value, s, ptab, &cx->lforms);
      } else {
        Scope sc(cx, e == 0 ? "gemm_inproj_raw" : "gemm_inproj_event", s);
        launch_gemm_split_blocks(cx->act[e][(l - 1) & 1], B * T, h->img.Wx16 + (size_t)(e * (depth - 1) + (l - 1)) * RV_WX16_SLOT, 4,
                                 h->img.bx2 + (size_t)(e * (depth - 1) + (l - 1)) * 2 * RV_G, cx->xw[e], 2 * RV_G, s);
      }
      a.x = cx->xw[e];
      a.dbg_ts = (e == 0 && l == 1 && cx->rec_ts_layer == 1) ? cx->rec_ts : nullptr;    // (RV_REC_STAMPS=2)
      Scope sc(cx, l == 0 ? "lstm_rec_event_l0" : (e == 0 ? "lstm_rec_raw_l1p" : "lstm_rec_event_l1p"), s);
      launch_lstm_rec_mx(a, 0, s, plan.rows8, &cx->lforms);
      a.dbg_ts = nullptr;
      continue;
    }
    if (l == 0) {
      a.x = x;
      for (int dr = 0; dr < 2; ++dr) { a.W[dr] = h->enc[e][0][dr].W; a.bias[dr] = h->enc[e][0][dr].b; }
      Scope sc(cx, e == 0 ? "lstm_rec_raw_l0" : "lstm_rec_event_l0", s);
      a.tail_wave = h->opt.tail_wave;
      a.dbg_ts = (e == 0 && cx->rec_ts_layer == 0) ? cx->rec_ts : nullptr;
      launch_lstm_rec(a, F, bt, s, &cx->lforms);
      a.dbg_ts = nullptr;
    } else {
      const float* in = cx->act[e][(l - 1) & 1];
      if (h->opt.fuse) {   // x . W + b on the matrix pipe inside the recurrence kernel: no K0 launch, no xw tensor
        a.x = in;
        a.dbg_role = h->dbg_role;
        for (int dr = 0; dr < 2; ++dr) {
          a.Wp[dr] = h->img.Wp + ((size_t)(e * (depth - 1) + (l - 1)) * 2 + dr) * RV_E * RV_G;
          a.Wh[dr] = h->opt.split_proj == 2 ? h->img.Wh + ((size_t)(e * (depth - 1) + (l - 1)) * 2 + dr) * wimg::WH_SLOT : nullptr;
          a.Wsb[dr] = h->opt.split_proj == 1 ? h->img.Wsb + ((size_t)(e * (depth - 1) + (l - 1)) * 2 + dr) * 3 * RV_E * RV_G : nullptr;
          a.bias[dr] = h->enc[e][l][dr].b;
        }
        a.dbg_ts = (e == 0 && l == 1 && cx->rec_ts_layer == 1) ? cx->rec_ts : nullptr;
        Scope sc(cx, e == 0 ? "lstm_rec_raw_l1p" : "lstm_rec_event_l1p", s);
        launch_lstm_rec_proj(a, bt, s, &cx->lforms);
        continue;
      }
      {   // both directions in ONE launch (same A): 2x the workgroups -> less round quantisation
        GemmArgs g{};
        g.A = in; g.lda = RV_E; g.ldb = RV_G; g.ldc = 2 * RV_G;
        g.M = B * T; g.N = RV_G; g.K = RV_E;
        g.Bm = h->enc[e][l][0].W; g.bias = h->enc[e][l][0].b; g.C = cx->xw[e];
        g.Bm1 = h->enc[e][l][1].W; g.bias1 = h->enc[e][l][1].b; g.C1 = cx->xw[e] + RV_G;
        g.xcd_remap = 1;
        Scope sc(cx, e == 0 ? "gemm_inproj_raw" : "gemm_inproj_event", s);
        launch_gemm_f32(g, false, s);
      }
      a.x = cx->xw[e];
      Scope sc(cx, e == 0 ? "lstm_rec_raw_l1p" : "lstm_rec_event_l1p", s);
      launch_lstm_rec(a, 0, bt, s, &cx->lforms);
    }
  }
}

void launch_decode_steps(SlabCtx* cx, const DecState& d, bool flash, hipStream_t s, bool profiled, FormLog* log) {
  RvContext* const h = cx->h;
  // A moves call whose steps take the single-pass attend, which never forms the alignments: the two-pass kernel runs first on the same
  // rows and leaves after its softmax with the step's records (DecState::moves_only); the step itself is the single-pass kernel's, so
  // the beam is what every other call's is
  // With debug_taps on, the alignment tap of such a call is the two-pass launch's -- the alignments its records are reduced from -- and
  // the single-pass kernel, which would store its raw scores to the same buffer, taps none
  DecState dm = d, ds = d;
  dm.moves_only = 1;
  const bool moves_aside = d.step_moves && flash;
  if (moves_aside) ds.step_align = nullptr;
  auto cells = [&](int step, bool prof) {
    for (int k = 0; k < d.depth; ++k) {
      if (h->rnn == RV_RNN_BIGRU) {
        const float* Wg = h->img.gWcatT + (size_t)k * RV_G * RV_E;
        if (prof) { Scope sc(cx, "dec_cell_gru"); launch_dec_cell_gru(d, k, Wg, k == 0 ? h->dec[0].W : nullptr, h->dec[k].b, step, s, log); }
        else launch_dec_cell_gru(d, k, Wg, k == 0 ? h->dec[0].W : nullptr, h->dec[k].b, step, s, log);
        continue;
      }
      const float* WcatT = h->img.WcatT + (size_t)k * RV_G * RV_E;
      if (prof) { Scope sc(cx, "dec_cell"); launch_dec_cell(d, k, WcatT, k == 0 ? h->dec[0].W : nullptr, h->dec[k].b, step, s); }
      else launch_dec_cell(d, k, WcatT, k == 0 ? h->dec[0].W : nullptr, h->dec[k].b, step, s);
    }
  };
  for (int step = 0; step < d.L - 1; ++step) {
    if (profiled) {
      cells(step, true);
      if (moves_aside) { Scope sc(cx, "dec_attend_moves"); launch_dec_attend(dm, h->img.WmemT, false, step, s, log); }
      { Scope sc(cx, "dec_attend"); launch_dec_attend(ds, h->img.WmemT, flash, step, s, log); }
    } else {
      cells(step, false);
      if (moves_aside) launch_dec_attend(dm, h->img.WmemT, false, step, s, log);
      launch_dec_attend(ds, h->img.WmemT, flash, step, s, log);
    }
  }
}

// The form of the one-launch persistent decode this call takes (dec_persist_form), or -1: the per-step kernels
int persist_form(const SlabCtx* cx, bool greedy, int W, int Tm, bool forced) {
  const RvContext* const h = cx->h;
  const bool gru = h->rnn == RV_RNN_BIGRU;
  if (gru && !(h->opt.gru_persist && h->gimg.built && cx->mem2)) return -1;      // (a GRU handle decodes per step unless option gru_persistent is on)
  if (!h->opt.persist || !h->opt.flash || cx->taps()) return -1;
  const RvConfig& c = h->cfg;
  if (forced && c.vocab >= RV_MAX_VOCAB) return -1;      // (a forced decode keeps a bias-only row behind the vocabulary's in the resident token table)
  // k_dec_persist_gru: one cell, everything but Bahdanau's scores on the matrix pipe -- no other GRU form exists to fall to
  if (gru) return c.dec_depth == 1 && h->opt.mx_att && h->opt.mx_cell ? dec_persist_form_gru(c.attention, greedy ? 1 : W, Tm, greedy) : -1;
  return dec_persist_form(c.attention, c.dec_depth, greedy ? 1 : W, Tm, greedy, h->opt.mx_att, h->opt.mx_cell);
}

// The plan of a validated call on context cx, under the handle's options as they are now
Plan plan_call(const SlabCtx* cx, const Call& call, const CallParts& res) {
  const RvContext* const h = cx->h;
  const Options& o = h->opt;
  const int form_B = res.form_B >= 0 ? res.form_B : call.B;      // a group takes the forms its first member would have got alone
  const bool gru = h->rnn == RV_RNN_BIGRU;                        // its one recurrence is the sixteen-chunk matrix-pipe kernel, whatever the slab
  const bool quiet = o.profile == 0 && !cx->taps();
  Plan p;
  p.wide = gru || wide_recurrence(h, form_B, call.T_r);
  p.rows8 = !gru && p.wide && rows8_wanted(h, form_B);
  p.fused_inproj = !gru && p.wide && !p.rows8 && fused_inproj_wanted(h, form_B);
  p.persist = persist_form(cx, call.greedy, call.W, call.T_r + call.T_e, res.labels != nullptr);
  // ---- setup_memory (basecaller.py:303): keys = (enc_output * mask) . W_mem.  The single-pass Luong attend never reads keys
  //      (score_t = values_t . (W_mem q)), and the persistent decode needs neither keys nor the per-step kernels; a moves call on the
  //      per-step kernels forms its alignments in the two-pass attend, beside the single-pass one where that runs the step
  p.flash = h->cfg.attention == RV_ATT_LUONG && o.flash && (call.greedy ? 1 : call.W) <= 5;      // wider beams: register budget -> two-pass
  p.keys = (!p.flash && p.persist < 0) || cx->taps() || (res.records() && p.persist < 0);
  // A window call: the default path gathers each chunk in the lane of its layer-0 recurrence; every other form -- the packed-FMA
  // recurrence, "lane_projection" 0, the per-step decode, taps, profiling, a group with "group_inplace" 0 -- runs unchanged behind
  // k_expand_windows, which writes the padded chunk tensors into the context's input buffers
  p.win_lane = call.windows && !gru && p.wide && (h->cfg.mode == RV_MODE_RAW || lane_layer0(h, 5, call.T_e)) && quiet && p.persist >= 0 &&
               !(cx->grp && !o.group_inplace);      // (k_gru_rec_mx gathers no windows: a GRU handle's window call runs behind k_expand_windows)
  // A slab graph: the default path only -- matrix-pipe recurrences + persistent decode, no profiling, no taps
  p.graphable = o.slab_graph && !gru && !call.windows && p.wide && !p.rows8 && p.persist >= 0 && quiet && !res.whole_beam && !res.labels && !res.records() &&
                !cx->ptaps() && !cx->rec_ts && !cx->dec_st.dbg_ts && cx->d_ptab;
  return p;
}

int record_slab(SlabCtx* cx, const Call& call, const CallParts& res, const Plan& plan, const void* const* ptab);
bool group_side_ev(const RvContext* h);

// The checks every call passes before anything is queued.  `ok` becomes the call with its effective lengths: T_r / T_e of an encoder
// the mode does not use are 0 there, and everything past this point works on `ok`
int validate_call(SlabCtx* cx, const Call& call, Call& ok) {
  RvContext* const h = cx->h; const RvConfig& c = h->cfg;
  if (!h->loaded) return fail(h, RV_ESTATE, "no weights loaded (call rv_load_weights first)");
  const bool use_raw = c.mode != RV_MODE_EVENT, use_ev = c.mode != RV_MODE_RAW;
  ok = call;
  if (!use_raw) ok.T_r = 0;
  if (!use_ev) ok.T_e = 0;
  const int B = ok.B, T_r = ok.T_r, T_e = ok.T_e, W = ok.W, L = ok.L;
  const float *raw = ok.raw, *ev = ok.ev;
  if (B < 0 || B > cx->cap) return fail(h, RV_EINVAL, "B=%d outside [0,%d]", B, cx->cap);      // (a group's context: its members' slabs together)
  if (use_raw && (T_r < 1 || T_r > c.max_raw_len)) return fail(h, RV_EINVAL, "T_r=%d outside [1,%d]", T_r, c.max_raw_len);
  if (use_ev && (T_e < 1 || T_e > c.max_event_len)) return fail(h, RV_EINVAL, "T_e=%d outside [1,%d]", T_e, c.max_event_len);
  if (W < 1 || W > c.max_beam || W > RV_MAX_BEAM) return fail(h, RV_EINVAL, "beam width %d outside [1,%d]", W, std::min(c.max_beam, RV_MAX_BEAM));
  if (L < 1 || L > c.max_output_len) return fail(h, RV_EINVAL, "max_output_len=%d outside [1,%d]", L, c.max_output_len);
  if (B > 0 && !ok.windows && ((use_raw && !raw) || (use_ev && !ev))) return fail(h, RV_EINVAL, "missing input pointer for this mode");   // (an empty device tensor has no address)
  if (T_r + T_e > 352) return fail(h, RV_EUNSUPPORTED, "attention memory of %d steps exceeds the 352 the decode kernel is built for", T_r + T_e);
  if (L > 64) return fail(h, RV_EUNSUPPORTED, "max_output_len %d exceeds 64", L);
  if (ok.dev_out && B > 0 && L > 1 && (!ok.tokens || !ok.out2)) return fail(h, RV_EINVAL, "null output pointer");
  // weight_parts 1: only the decode whose every weight comes from an image of a rounded tensor -- the persistent decode of one cell
  // with Luong attention and the cell product on the matrix pipe (ATT 3: Wkp16 / Wmp16, Wc16, Wl16).  The per-step kernels and the
  // other persistent forms read the cell kernel, the attention layer or the output layer from the blob, which holds them unrounded
  if (h->opt.parts_loaded == 1 && (c.dec_depth != 1 || persist_form(cx, ok.greedy, W, T_r + T_e, ok.forced != nullptr) != 3))
    return fail(h, RV_EUNSUPPORTED, "weight_parts 1 serves the persistent decode of one decoder cell with Luong attention and the cell product on the matrix "
                "pipe only (options persistent_decode, flash_attend, matrix_attention, matrix_cell at 1, debug_taps 0): this call would read unrounded weights");
  return RV_OK;
}

// Everything of a call up to (not including) the wait for the stream: launches and the D2H copies into pinned staging.
int enqueue(SlabCtx* cx, const Call& stated, const CallParts& res) {
  RvContext* const h = cx->h; const RvConfig& c = h->cfg;
  if (cx->pend.busy) return fail(h, RV_ESTATE, "this context still holds an uncollected call");
  const bool use_raw = c.mode != RV_MODE_EVENT, use_ev = c.mode != RV_MODE_RAW;
  Call call;
  TRY(validate_call(cx, stated, call));
  const int B = call.B, T_r = call.T_r, T_e = call.T_e, W = call.W, L = call.L;
  const bool greedy = call.greedy, dev_out = call.dev_out, calls = call.lut != nullptr;
  HIPCHK(h, hipSetDevice(c.device));
  cx->lB = B; cx->fact.lW = W; cx->lL = L; cx->lgreedy = greedy; cx->lTm = T_r + T_e; cx->ltaps = cx->taps(); cx->lptaps = cx->ptaps();
  cx->lmoves = res.records() ? 1 : 0;
  if (cx->own()) h->lS = 0;
  cx->lforms.n = 0; cx->lforms.full = false; cx->lforms_ok = 1;
  cx->pend = SlabCtx::PendingCall{};
  cx->pend.busy = true; cx->pend.greedy = greedy; cx->pend.dev_out = dev_out; cx->pend.calls = calls; cx->pend.all = res.whole_beam; cx->pend.moves = res.moves; cx->pend.cmoves = res.call_moves;
  cx->pend.stitch = stated.stitch != nullptr;
  cx->pend.B = B; cx->pend.steps = std::max(L - 1, 0); cx->pend.V = c.vocab; cx->pend.Wd = greedy ? 1 : W;
  if (B == 0 || L <= 1) {
    cx->pend.trivial = true;
    if (res.whole_beam && dev_out && B > 0) {      // nothing is launched: the initial state goes to the caller's device buffers by plain copies
      std::vector<float> lp((size_t)B * W, -INFINITY);
      for (int b = 0; b < B; ++b) lp[(size_t)b * W] = 0.f;
      if (res.beams.log_probs) HIPCHK(h, hipMemcpy(res.beams.log_probs, lp.data(), sizeof(float) * lp.size(), hipMemcpyHostToDevice));
      if (res.beams.lengths) HIPCHK(h, hipMemset(res.beams.lengths, 0, sizeof(int32_t) * (size_t)B * W));
    }
    return RV_OK;
  }

  // From here on `call` names device memory throughout: the inputs the encoders read and the outputs the finalize kernel writes
  // (dev_in / dev_out still say whose they are, so which copies the recording adds)
  hipStream_t s = cx->stream;
  if (!call.dev_in) {   // host -> pinned staging (CPU memcpy); the H2D copies are part of the slab's stream work (record_slab)
    if (use_raw) { memcpy(cx->pin_raw, call.raw, sizeof(float) * B * T_r); call.raw = cx->d_raw; }
    if (use_ev) { memcpy(cx->pin_ev, call.ev, sizeof(float) * B * T_e * 5); call.ev = cx->d_ev; }
  }
  if (!dev_out || !call.tokens) call.tokens = cx->out_tokens;
  if (!dev_out || !call.out2) call.out2 = cx->out2;

  const Plan plan = plan_call(cx, call, res);
  if (call.windows) {
    // The table goes to this context's pinned staging now (a group's rows are there already: submit_group); its device copy is the first
    // thing the recording queues (stage_inputs)
    if (call.windows != cx->pin_win) memcpy(cx->pin_win, call.windows, sizeof(RecWindow) * (size_t)B);
    call.windows = cx->d_win;
    call.win_expand = !plan.win_lane;
    if (call.win_expand) { call.raw = use_raw ? cx->d_raw : nullptr; call.ev = use_ev ? cx->d_ev : nullptr; }
  }

  // ---- one hipGraph per slab context and call shape (option "slab_graph"): the default path replays as ONE hipGraphLaunch instead
  // of ten launches (a submit's host time is what the GPU waits for whenever the slabs in flight finish together).  All kernel arguments
  // are frozen at capture; the caller's addresses of THIS call go through the pointer table (mapped pinned memory, written here, read by
  // the kernels).
  if (cx->graph_gen != h->opt.gen) {            // an option or the weights changed since the capture: frozen arguments may be stale
    for (auto& kv : cx->slab_graphs) hipGraphExecDestroy(kv.second.exec);
    cx->slab_graphs.clear();
    cx->graph_gen = h->opt.gen;
  }
  if (!plan.graphable) return record_slab(cx, call, res, plan, nullptr);
  cx->lforms_ok = 0;                             // (a slab graph replays without the host launchers: "kernel_forms" answers RV_ESTATE)
  cx->pin_ptab[RV_PTAB_RAW] = call.raw; cx->pin_ptab[RV_PTAB_EVENT] = call.ev; cx->pin_ptab[RV_PTAB_TOKENS] = call.tokens; cx->pin_ptab[RV_PTAB_OUT2] = call.out2;
  SlabKey key{B, T_r, T_e, W, L, (greedy ? 1 : 0) | (calls ? 2 : 0) | (call.dev_in ? 0 : 4) | (dev_out ? 0 : 8) | (plan.fused_inproj ? 16 : 0), 0};
  if (calls) memcpy(&key.lut, call.lut, std::min<size_t>(sizeof key.lut, (size_t)c.vocab));
  auto it = cx->slab_graphs.find(key);
  if (it == cx->slab_graphs.end()) {
    if (cx->slab_graphs.size() >= 16) {          // bound the cache (callers with ever-changing slab shapes)
      for (auto& kv : cx->slab_graphs) hipGraphExecDestroy(kv.second.exec);
      cx->slab_graphs.clear();
    }
    hipGraph_t graph = nullptr;
    HIPCHK(h, hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal));
    const int rc = record_slab(cx, call, res, plan, cx->d_ptab);
    const hipError_t ce = hipStreamEndCapture(s, &graph);      // (always: the stream must leave capture mode whatever record_slab said)
    if (rc != RV_OK) { if (graph) hipGraphDestroy(graph); return rc; }
    HIPCHK(h, ce);
    SlabCtx::SlabGraph g;
    const hipError_t ie = hipGraphInstantiate(&g.exec, graph, nullptr, nullptr, 0);
    hipGraphDestroy(graph);
    HIPCHK(h, ie);
    g.fact = cx->fact;
    it = cx->slab_graphs.emplace(key, g).first;
  }
  const SlabCtx::SlabGraph& g = it->second;
  cx->fact = g.fact;
  HIPCHK(h, hipGraphLaunch(g.exec, s));
  return RV_OK;
}

// One recording of a slab (record_slab): the call as enqueue() resolved it, and what the phases below hand on to each other
struct Slab {
  const Call& call;
  const CallParts& res;
  const Plan& plan;
  const void* const* ptab;      // non-null: the call is being captured into a slab graph
  int Tm, steps;
  DecState d{};                 // the whole slab's decode ...
  int nsplit = 1;
  DecState part[4];             // ... and its sub-slabs (one part unless the per-step decode splits)
  DecParts parts{};
};

// Phase 1 of a recording: the inputs of a host caller, pinned staging -> device
int stage_inputs(SlabCtx* cx, const Slab& sl) {
  RvContext* const h = cx->h; const RvConfig& c = h->cfg;
  const bool use_raw = c.mode != RV_MODE_EVENT, use_ev = c.mode != RV_MODE_RAW;
  const int B = sl.call.B, T_r = sl.call.T_r, T_e = sl.call.T_e;
  hipStream_t s = cx->stream;
  if (!sl.call.dev_in) {   // pinned staging -> device
    if (use_raw) HIPCHK(h, hipMemcpyAsync(cx->d_raw, cx->pin_raw, sizeof(float) * B * T_r, hipMemcpyHostToDevice, s));
    if (use_ev) HIPCHK(h, hipMemcpyAsync(cx->d_ev, cx->pin_ev, sizeof(float) * B * T_e * 5, hipMemcpyHostToDevice, s));
  }
  if (sl.call.windows) {   // a window call: its table, 24 bytes per chunk, behind the uploads of the reads it names
    if (h->ev_put) HIPCHK(h, hipStreamWaitEvent(s, h->ev_put, 0));
    HIPCHK(h, hipMemcpyAsync(cx->d_win, cx->pin_win, sizeof(RecWindow) * (size_t)B, hipMemcpyHostToDevice, s));
    if (sl.call.win_expand) {
      Scope sc(cx, "expand_windows");
      h->win_expands += 1;
      launch_expand_windows(cx->d_win, B, use_raw ? cx->d_raw : nullptr, T_r, use_ev ? cx->d_ev : nullptr, T_e, c.padding_value, s);
    }
  }
  return RV_OK;
}

// Phase 2: the input mask and the two encoders, on one of three stream arrangements
int record_encoders(SlabCtx* cx, const Slab& sl) {
  RvContext* const h = cx->h; const RvConfig& c = h->cfg;
  const bool use_raw = c.mode != RV_MODE_EVENT, use_ev = c.mode != RV_MODE_RAW;
  const int B = sl.call.B, T_r = sl.call.T_r, T_e = sl.call.T_e, Tm = sl.Tm;
  const float *xr = sl.call.raw, *xe = sl.call.ev;
  const void* const* ptab = sl.ptab;
  const RecWindow* win = sl.call.win_expand ? nullptr : sl.call.windows;      // (only the matrix-pipe layer 0 with the projection in the lane takes windows: enqueue)
  hipStream_t s = cx->stream;
  // ---- _encode_input (basecaller.py:395-416)
  // The mask is first read by the memory set-up / the decode: it runs on a side stream beside the encoders instead of in front
  // of them (profiling modes keep it on the main stream so that its events pair up).
  // (with several slabs in flight the other slabs fill the chip: one stream per context then, no fork / join)
  // The matrix-pipe layer-0 kernels write it themselves (they read every input sample anyway): no launch at all then.
  const bool wide = sl.plan.wide;
  const bool mask_aside = !wide && (h->opt.profile == 0 || h->opt.profile == 3) && h->inflight_hint <= 1 && cx->own();
  if (mask_aside) {
    hipStream_t sm = side_stream(cx, 2);
    HIPCHK(h, hipEventRecord(cx->ev_fork, s));
    HIPCHK(h, hipStreamWaitEvent(sm, cx->ev_fork, 0));     // inputs (H2D copies on s) are in place
    launch_input_mask(xr, xe, B, T_r, T_e, c.padding_value, cx->mask, sm);
    HIPCHK(h, hipEventRecord(cx->ev_join[2], sm));
  } else if (!wide) {
    Scope sc(cx, "input_mask"); launch_input_mask(xr, xe, B, T_r, T_e, c.padding_value, cx->mask, s);
  }
  // The two encoders are independent until the time-axis concat (basecaller.py:400-405).
  const bool side_ev = use_raw && use_ev && h->opt.side_ev && c.enc_depth > 1 && !h->opt.fuse;   // (nothing MFMA-bound to hide under once the projection is fused)
  if (side_ev) {
    // raw layer 0 alone (every recurrence workgroup needs a whole CU); then the short event chain on a side stream
    // UNDER the raw encoder's input-projection GEMM: a recurrence workgroup (2 x 168 VGPRs per SIMD, VALU-bound) and a
    // GEMM workgroup (144 registers, MFMA-bound) fit on one CU together.
    hipStream_t sev = side_stream(cx, 0);
    run_encoder(cx, sl.plan, 0, xr, 1, B, T_r, Tm, 0, s, 0, 1);
    HIPCHK(h, hipEventRecord(cx->ev_fork, s));
    HIPCHK(h, hipStreamWaitEvent(sev, cx->ev_fork, 0));
    run_encoder(cx, sl.plan, 1, xe, 5, B, T_e, Tm, T_r, sev);
    run_encoder(cx, sl.plan, 0, xr, 1, B, T_r, Tm, 0, s, 1);
    HIPCHK(h, hipEventRecord(cx->ev_join[0], sev));
    HIPCHK(h, hipStreamWaitEvent(s, cx->ev_join[0], 0));
  } else if (wide && use_raw && use_ev && !ptab && h->opt.profile == 0 &&
             ((h->inflight_hint <= 1 && h->opt.side_ev) || (cx->grp && group_side_ev(h)))) {
    // One isolated slab on the matrix-pipe form: every encoder launch is 2 x ceil(B / 16) workgroups (32 of the chip's 256 CUs at B = 256), so
    // the event encoder's chain (four launches, ~0.15 ms at the C3 shape) runs on a side stream BESIDE the raw encoder's instead of in front of
    // it: the synchronous call's latency drops by that much.  (With several slabs in flight the other slabs fill the chip: one stream per
    // context then, no fork / join.)  The two encoders write disjoint time ranges of enc_out and of the mask and use their own xw / act / state
    // buffers: results are identical.
    // A group of coalesced slabs forks the same way where the queues allow it (group_side_ev): with two groups in flight each one's next
    // launch waits for its whole chain, and the event launches (2 x ceil(B / 16) workgroups: 160 of 256 CUs for five C3 slabs) need not be
    // links of it.
    hipStream_t sev = side_stream(cx, 0);
    HIPCHK(h, hipEventRecord(cx->ev_fork, s));
    HIPCHK(h, hipStreamWaitEvent(sev, cx->ev_fork, 0));       // inputs (H2D copies on s) are in place
    run_encoder(cx, sl.plan, 1, xe, 5, B, T_e, Tm, T_r, sev, 0, 1 << 30, nullptr, win);
    HIPCHK(h, hipEventRecord(cx->ev_join[0], sev));
    run_encoder(cx, sl.plan, 0, xr, 1, B, T_r, Tm, 0, s, 0, 1 << 30, nullptr, win);
    HIPCHK(h, hipStreamWaitEvent(s, cx->ev_join[0], 0));
  } else {
    if (use_ev) run_encoder(cx, sl.plan, 1, xe, 5, B, T_e, Tm, T_r, s, 0, 1 << 30, ptab, win);
    if (use_raw) run_encoder(cx, sl.plan, 0, xr, 1, B, T_r, Tm, 0, s, 0, 1 << 30, ptab, win);
  }

  if (mask_aside) HIPCHK(h, hipStreamWaitEvent(s, cx->ev_join[2], 0));
  return RV_OK;
}

// Phase 3: the key GEMM where the call's attend or a tap needs it (Plan::keys)
int record_keys(SlabCtx* cx, const Slab& sl) {
  RvContext* const h = cx->h;
  const int B = sl.call.B, Tm = sl.Tm;
  hipStream_t s = cx->stream;
  cx->fact.lflash = sl.plan.flash ? 1 : 0;
  cx->fact.lkeys = sl.plan.keys ? 1 : 0;
  if (sl.plan.keys) {
    GemmArgs g{};
    g.A = cx->enc_out; g.lda = RV_E; g.Bm = h->W_mem; g.ldb = RV_U; g.C = cx->keys; g.ldc = RV_U;
    g.M = B * Tm; g.N = RV_U; g.K = RV_E; g.row_mask = cx->mask;
    Scope sc(cx, "gemm_keys");
    launch_gemm_f32(g, false, s);
  }
  return RV_OK;
}

// A debug-tap buffer of at least `need` floats
int grow_tap_buffer(SlabCtx* cx, float** buf, size_t* cap, size_t need) {
  RvContext* const h = cx->h;
  if (need <= *cap) return RV_OK;
  if (*buf) hipFree(*buf);
  *buf = nullptr; *cap = 0;
  for (auto& kv : cx->graphs) hipGraphExecDestroy(kv.second);   // captured args hold the old pointer
  cx->graphs.clear();
  HIPCHK(h, hipMalloc((void**)buf, need * sizeof(float)));
  *cap = need;
  return RV_OK;
}

// Phase 4: the decode's arguments (sl.d) and the debug-tap buffers
int fill_dec_state(SlabCtx* cx, Slab& sl) {
  RvContext* const h = cx->h; const RvConfig& c = h->cfg;
  const int B = sl.call.B, W = sl.call.W, L = sl.call.L, Tm = sl.Tm, V = c.vocab, steps = sl.steps;
  const bool greedy = sl.call.greedy, calls = sl.call.lut != nullptr;
  hipStream_t s = cx->stream;
  // ---- decode loop
  DecState& d = sl.d;
  d = cx->dec_st;
  d.B = B; d.W = greedy ? 1 : W; d.Tm = Tm; d.V = V; d.L = L;
  d.greedy = greedy; d.attention = c.attention;
  d.forced = sl.res.labels;
  d.start_token = c.start_token; d.end_token = c.end_token; d.pad_token = c.pad_token;
  d.attend_threads = h->opt.att_nt;
  d.keys = cx->keys; d.values = cx->enc_out; d.mask = cx->mask;
  d.W_att = h->W_att; d.W_fc = h->W_fc; d.b_fc = h->b_fc; d.W_q = h->W_q; d.v_att = h->v_att;
  d.call_bases = nullptr; d.call_probs = nullptr; d.call_len = nullptr;
  if (calls) {
    d.call_bases = cx->d_bases; d.call_probs = cx->d_probs; d.call_len = cx->d_clen;
    for (int v = 0; v < RV_MAX_VOCAB; ++v) d.lut[v] = v < V ? sl.call.lut[v] : 0;
  }
  const size_t need = (size_t)steps * B * d.W * Tm;      // alignments of every step
  if (cx->taps()) {
    TRY(grow_tap_buffer(cx, &cx->step_align, &cx->step_align_cap, need));
    d.step_align = cx->step_align;
  } else {
    d.step_align = nullptr;
    if (!greedy && !cx->ptaps()) d.step_logits = nullptr;
  }
  d.persist_align = nullptr;
  if (cx->ptaps()) {
    TRY(grow_tap_buffer(cx, &cx->palign, &cx->palign_cap, need));
    // NaN everywhere first: a step the kernel does not record is never read as a stale value of an earlier call
    if (need) HIPCHK(h, hipMemsetAsync(cx->palign, 0xff, need * sizeof(float), s));
    d.persist_align = cx->palign;
  }
  d.step_moves = sl.res.records() ? cx->d_step_moves : nullptr;
  d.Tr = sl.call.T_r;      // (effective lengths: T_m in raw mode, 0 in event mode)
  d.moves_only = 0;
  return RV_OK;
}

// ... then which decode runs (lpersist), its sub-slabs (sl.part, sl.parts) and, for the per-step kernels, their initial state
int split_decode(SlabCtx* cx, Slab& sl) {
  RvContext* const h = cx->h; const RvConfig& c = h->cfg;
  const int B = sl.call.B, Tm = sl.Tm, V = c.vocab, steps = sl.steps, persist_att = sl.plan.persist;
  const bool greedy = sl.call.greedy;
  hipStream_t s = cx->stream;
  DecState& d = sl.d;
  DecState* part = sl.part;
  DecParts& parts = sl.parts;
  int& nsplit = sl.nsplit;
  const int N = B * d.W;
  // The slab decodes as `nsplit` independent sub-slabs on concurrent streams (inside one hipGraph):
  // while one sub-slab is in its HBM-bound attention sweep another runs its latency-bound cell /
  // output / beam phases.  Chunks never interact, and a sub-slab that finishes early is extended by
  // k_dec_finalize exactly as the reference's whole-slab loop would (beam search only; greedy rows
  // keep sampling after their end token, so greedy decodes as one piece).
  nsplit = (greedy || cx->taps() || B < 64) ? 1 : std::min(std::max(h->opt.split, 1), 4);
  d.chunk_steps = nullptr;
  d.persist_att = persist_att;
  d.Wc16 = h->img.Wc16; d.mx_cdescale = h->scales.cdescale; d.Wl16 = h->img.Wl16; d.mx_ldescale = h->scales.ldescale;
  d.Wq16 = h->img.Wq16; d.mx_qdescale = h->scales.qdescale; d.W1c16 = h->img.W1c16; d.mx_c1descale = h->scales.c1descale;
  const bool persist = persist_att >= 0;
  if (persist && h->rnn == RV_RNN_BIGRU) {      // k_dec_persist_gru: the folded GRU images under the LSTM forms' names
    const GruPersistDev& gi = h->gimg;
    d.Wc16 = gi.gWc16; d.mx_cdescale = gi.scales.cdescale; d.Wl16 = gi.gWl16; d.mx_ldescale = gi.scales.ldescale;
    d.Wq16 = gi.gWq16; d.mx_qdescale = gi.scales.qdescale;
  }
  cx->fact.lpersist = persist ? 1 : 0;
  cx->fact.lmem2_stale = 0;
  if (persist) { nsplit = 1; d.chunk_steps = cx->d_chunk_steps; }
  cx->fact.lsplit = nsplit;
  if (!persist) {
    for (int k = 0; k < d.depth; ++k) {     // get_initial_state: all zeros (basecaller.py:305); the persistent kernel keeps state in LDS
      HIPCHK(h, hipMemsetAsync(d.xh + k * d.ls_xh, 0, sizeof(float) * N * RV_E, s));
      if (h->rnn == RV_RNN_BILSTM) HIPCHK(h, hipMemsetAsync(d.c + k * d.ls_c, 0, sizeof(float) * N * RV_U, s));      // (a GRU cell has no c)
    }
  }
  const int Wd = d.W;
  parts = DecParts{};
  parts.n = nsplit; parts.steps = steps; parts.S_dev = d.S_dev; parts.S_host = d.S_host;
  for (int g = 0; g < nsplit; ++g) {
    const size_t b0 = (size_t)B * g / nsplit, b1 = (size_t)B * (g + 1) / nsplit;
    DecState& p = part[g];
    p = d;
    p.part = g; p.B = (int)(b1 - b0);
    if (p.call_bases) { p.call_bases += b0 * steps; p.call_probs += b0 * steps; p.call_len += b0; }
    p.keys += b0 * Tm * RV_U; p.values += b0 * Tm * RV_E; p.mask += b0 * Tm;
    p.xh += b0 * Wd * RV_E; p.z += b0 * Wd * RV_G;
    p.c += b0 * Wd * RV_U; p.c_new += b0 * Wd * RV_U; p.h_new += b0 * Wd * RV_U;
    p.tok += b0 * Wd; p.log_probs += b0 * Wd; p.finished += b0 * Wd; p.lengths += b0 * Wd;
    p.step_ids += (size_t)steps * Wd * b0; p.parent_ids += (size_t)steps * Wd * b0; p.step_scores += (size_t)steps * Wd * b0;
    if (p.step_logits) p.step_logits += (size_t)steps * Wd * V * b0;
    if (p.step_align) p.step_align += (size_t)steps * Wd * Tm * b0;
    if (p.persist_align) p.persist_align += (size_t)steps * Wd * Tm * b0;
    if (p.step_moves) p.step_moves += (size_t)steps * Wd * RV_MOVE_COLS * b0;
    p.nfin = d.nfin + g * (c.max_output_len + 1);
    parts.nfin[g] = p.nfin; parts.B[g] = p.B;
    if (!persist) launch_dec_init(p, s);
  }
  return RV_OK;
}

// Phase 5: the persistent decode -- the whole loop in one launch, behind the projection of its attention memory where it does not project its own
int decode_persist(SlabCtx* cx, Slab& sl) {
  RvContext* const h = cx->h;
  const int B = sl.call.B, Tm = sl.Tm, V = h->cfg.vocab, persist_att = sl.plan.persist;
  const bool greedy = sl.call.greedy;
  hipStream_t s = cx->stream;
  DecState& d = sl.d;
  DecState* part = sl.part;
  DecParts& parts = sl.parts;
  part[0] = d; part[0].part = 0; parts.n = 1;
  if (greedy) HIPCHK(h, hipMemsetAsync(d.nfin, 0, 2 * sizeof(int), s));   // chunks-finished count and latest first-finish step
  // The default form (Luong, one cell, everything on the matrix pipe) takes enc_out and projects each chunk's rows in its own
  // prologue, with the split GEMM's arithmetic (decode.hip, persist_project_memory); every other form reads the GEMM's mem2
  const bool fused_mem = h->opt.fused_mem && h->opt.split_proj && persist_att == 3 && d.depth == 1;
  cx->fact.lmem2_stale = fused_mem && !cx->ptaps();
  const bool gru = h->rnn == RV_RNN_BIGRU;
  const wimg::ImageScales& scales = gru ? h->gimg.scales : h->scales;
  const float* Wmp = gru ? h->gimg.gWmp : h->img.Wmp;
  const uint16_t* Wmp16 = gru ? h->gimg.gWmp16 : h->img.Wmp16;
  d.enc_rows = nullptr; d.Wmp16 = Wmp16; d.Wkp16 = gru ? h->gimg.gWkp16 : h->img.Wkp16; d.mem_tap = nullptr;
  if (fused_mem) {
    d.enc_rows = cx->enc_out; d.mem_tap = cx->ptaps() ? cx->mem2 : nullptr;
  } else {   // attention memory in the form the persistent decode keeps on chip: [keys | U'] = enc_out . [W_mem | A_c]
    GemmArgs g{};
    g.A = cx->enc_out; g.lda = RV_E; g.Bm = Wmp; g.ldb = RV_E; g.C = cx->mem2; g.ldc = RV_E;
    g.M = B * Tm; g.N = RV_E; g.K = RV_E;
    g.xcd_remap = 1;
    Scope sc(cx, "gemm_memory");
    if (h->opt.split_proj) launch_gemm_mem_split(cx->enc_out, B * Tm, Wmp16, cx->mem2, s);
    else launch_gemm_f32(g, false, s);
  }
  d.values = cx->mem2; part[0].values = cx->mem2;
  d.mx_kscale = scales.kscale; d.mx_kdescale = std::ldexp(1.0f, -14) / scales.kscale;
  d.mx_uscale = scales.uscale; d.mx_udescale = std::ldexp(1.0f, -14) / scales.uscale;
  if (gru) {
    Scope sc(cx, "dec_persist_gru", nullptr, true);
    launch_dec_persist_gru(d, h->gimg.gWtok, h->gimg.gbdec, s, &cx->lforms);
    return RV_OK;
  }
  const bool p1 = h->opt.parts_loaded == 1 && h->opt.one_part && persist_att == 3 && d.depth == 1;
  Scope sc(cx, "dec_persist", nullptr, true);
  launch_dec_persist(d, d.depth > 1 ? h->dec[0].W + (size_t)V * RV_G : h->img.Wcat2, h->dec[0].W, h->dec[0].b,
                     d.depth > 1 ? h->dec[1].W : nullptr, d.depth > 1 ? h->dec[1].b : nullptr, h->img.Nh, s, &cx->lforms,
                     p1 ? h->img.Wc16p1 : nullptr, p1 ? h->img.Wl16p1 : nullptr);
  return RV_OK;
}

// The per-step launches of every sub-slab: part 0 on the context's stream, the others forked onto side streams and joined again
int fork_decode_steps(SlabCtx* cx, const Slab& sl, bool profiled, FormLog* log) {
  RvContext* const h = cx->h;
  const int nsplit = sl.nsplit;
  hipStream_t s = cx->stream;
  for (int g = 1; g < nsplit; ++g) {
    HIPCHK(h, hipEventRecord(cx->ev_fork, s));
    HIPCHK(h, hipStreamWaitEvent(side_stream(cx, g - 1), cx->ev_fork, 0));
  }
  for (int g = 0; g < nsplit; ++g) launch_decode_steps(cx, sl.part[g], sl.plan.flash, g == 0 ? s : side_stream(cx, g - 1), profiled && nsplit == 1, log);
  for (int g = 1; g < nsplit; ++g) {
    HIPCHK(h, hipEventRecord(cx->ev_join[g - 1], side_stream(cx, g - 1)));
    HIPCHK(h, hipStreamWaitEvent(s, cx->ev_join[g - 1], 0));
  }
  return RV_OK;
}

// FormLog::merge (inline, common.h) has always left this file out of line, and so among the library's dynamic symbols: the list stays
// what it was whatever the inliner makes of the one call below
[[gnu::used]] void (FormLog::*const formlog_merge_out_of_line)(const FormLog&) = &FormLog::merge;

// Phase 6: the per-step decode -- a replay of the decode graph of this shape (captured on its first use), or direct launches
int decode_steps(SlabCtx* cx, Slab& sl) {
  RvContext* const h = cx->h;
  const int B = sl.call.B, L = sl.call.L, Tm = sl.Tm;
  const bool greedy = sl.call.greedy;
  hipStream_t s = cx->stream;
  DecState& d = sl.d;
  DecState* part = sl.part;
  DecParts& parts = sl.parts;
  int& nsplit = sl.nsplit;
  // (a forced decode and a moves call launch their steps without replay: the label and the records pointers are no part of the key)
  if (h->opt.graph && h->opt.profile != 2 && !d.forced && !d.step_moves) {
    GraphKey key{B, d.W, Tm, L, greedy ? 1 : 0, cx->taps() * 2 + (sl.plan.flash ? 1 : 0) + 4 * h->opt.att_nt + 4096 * (d.step_logits ? 1 : 0) + 8192 * (d.persist_align ? 1 : 0), nsplit};   // every captured pointer that can change is in the key
    auto it = cx->graphs.find(key);
    if (it == cx->graphs.end()) {
      if (cx->graphs.size() >= 32) {      // bound the cache (callers with ever-changing slab shapes)
        for (auto& kv : cx->graphs) hipGraphExecDestroy(kv.second);
        cx->graphs.clear();
        cx->graph_forms.clear();
      }
      FormLog& gforms = cx->graph_forms[key];
      gforms.n = 0; gforms.full = false;
      hipGraph_t graph = nullptr;
      HIPCHK(h, hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal));
      const int rc = fork_decode_steps(cx, sl, false, &gforms);
      hipError_t ce = hipStreamEndCapture(s, &graph);
      if (rc != RV_OK) return rc;
      HIPCHK(h, ce);
      hipGraphExec_t exec = nullptr;
      HIPCHK(h, hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0));
      hipGraphDestroy(graph);
      it = cx->graphs.emplace(key, exec).first;
    }
    cx->lforms.merge(cx->graph_forms[key]);      // the launches of the graph's capture: it replays those
    Scope sc(cx, "decode_graph", nullptr, true);
    HIPCHK(h, hipGraphLaunch(it->second, s));
  } else {
    if (h->opt.profile == 2) nsplit = 1, parts.n = 1;     // per-kernel events need one stream
    if (nsplit == 1) { part[0] = d; part[0].part = 0; part[0].nfin = d.nfin; parts.nfin[0] = d.nfin; parts.B[0] = B; launch_dec_init(part[0], s); }
    TRY(fork_decode_steps(cx, sl, h->opt.profile == 2, &cx->lforms));
  }
  return RV_OK;
}

// Phase 7: the outputs of every sub-slab from its beam records (k_dec_finalize, or k_dec_finalize_beams for the whole beam: never a
// group, never captured), then the scores of a forced decode
int finalize_and_score(SlabCtx* cx, const Slab& sl) {
  RvContext* const h = cx->h; const RvConfig& c = h->cfg;
  const int B = sl.call.B, L = sl.call.L, V = c.vocab, steps = sl.steps, Wd = sl.d.W;
  const bool greedy = sl.call.greedy;
  int32_t* tk = sl.call.tokens;
  float* o2 = sl.call.out2;
  hipStream_t s = cx->stream;
  const DecState& d = sl.d;
  const DecParts& parts = sl.parts;
  {
    Scope sc(cx, sl.res.whole_beam ? "dec_finalize_beams" : "dec_finalize");
    if (sl.plan.persist < 0) launch_dec_reduce_steps(parts, s);
    for (int g = 0; g < parts.n; ++g) {
      const size_t b0 = parts.n == 1 ? 0 : (size_t)B * g / parts.n;      // the sub-slab's first chunk
      if (sl.res.whole_beam) {
        BeamsOut o = sl.res.beams;
        o.tokens += b0 * steps * Wd; o.scores += b0 * steps * Wd;
        if (o.path_scores) o.path_scores += b0 * steps * Wd;
        if (o.log_probs) o.log_probs += b0 * Wd;
        if (o.lengths) o.lengths += b0 * Wd;
        launch_dec_finalize_beams(sl.part[g], o, s);
      } else {
        launch_dec_finalize(sl.part[g], tk + b0 * steps, o2 + b0 * steps * (greedy ? V : 1), s, sl.ptab,      // (ptab: persistent decode only, one part)
                            sl.plan.persist >= 0 ? sl.res.members : nullptr);
      }
    }
  }
  if (sl.res.moves) {      // behind k_dec_finalize_beams, which left S for every part
    Scope sc(cx, "dec_finalize_moves");
    for (int g = 0; g < parts.n; ++g) {
      const size_t off = (parts.n == 1 ? 0 : (size_t)B * g / parts.n) * steps * Wd;
      MovesOut o = sl.res.moves_out;
      if (o.raw_pos) o.raw_pos += off;
      if (o.raw_mass) o.raw_mass += off;
      if (o.event_pos) o.event_pos += off;
      if (o.event_mass) o.event_mass += off;
      if (o.peak) o.peak += off;
      if (o.peak_weight) o.peak_weight += off;
      launch_dec_finalize_moves(sl.part[g], o, s);
    }
  }
  if (sl.res.call_moves || sl.res.forced_moves) {      // [B,L-1]: behind k_dec_finalize, which left the tokens and S of every part
    Scope sc(cx, sl.res.call_moves ? "dec_finalize_calls_moves" : "forced_moves");
    for (int g = 0; g < parts.n; ++g) {
      const size_t off = (parts.n == 1 ? 0 : (size_t)B * g / parts.n) * steps;
      MovesOut o = sl.res.moves_out;
      if (o.raw_pos) o.raw_pos += off;
      if (o.raw_mass) o.raw_mass += off;
      if (o.event_pos) o.event_pos += off;
      if (o.event_mass) o.event_mass += off;
      if (o.peak) o.peak += off;
      if (o.peak_weight) o.peak_weight += off;
      if (sl.res.call_moves) launch_dec_finalize_calls_moves(sl.part[g], tk + off, o, s);
      else launch_forced_moves(sl.part[g], o, s);
    }
  }
  if (d.forced) {      // the forced decode's labels target[:, 1:] against the logits the finalize kernel just wrote
    ScoreArgs a = sl.res.score;
    a.logits = o2; a.labels = d.forced + 1; a.label_stride = L; a.B = B; a.S = steps; a.V = V; a.pad_token = c.pad_token; a.pred = nullptr;
    Scope sc(cx, "score_tokens");
    launch_score_tokens(a, s);
  }
  return RV_OK;
}

// Phase 8: the results of a host caller, device -> pinned staging
int stage_outputs(SlabCtx* cx, const Slab& sl) {
  RvContext* const h = cx->h;
  const int B = sl.call.B, V = h->cfg.vocab, steps = sl.steps, Wd = sl.d.W;
  const bool greedy = sl.call.greedy, dev_out = sl.call.dev_out, calls = sl.call.lut != nullptr;
  hipStream_t s = cx->stream;
  // (S reaches the host through d.S_host: the finalize / reduce kernel stores it straight into the mapped pinned word)
  if (sl.res.whole_beam && !dev_out) {
    const BeamsOut &o = sl.res.beams, &p = cx->pin_beams;
    const size_t n = (size_t)B * steps * Wd, nb = (size_t)B * Wd;
    HIPCHK(h, hipMemcpyAsync(p.tokens, o.tokens, sizeof(int32_t) * n, hipMemcpyDeviceToHost, s));
    HIPCHK(h, hipMemcpyAsync(p.scores, o.scores, sizeof(float) * n, hipMemcpyDeviceToHost, s));
    if (o.path_scores) HIPCHK(h, hipMemcpyAsync(p.path_scores, o.path_scores, sizeof(float) * n, hipMemcpyDeviceToHost, s));
    if (o.log_probs) HIPCHK(h, hipMemcpyAsync(p.log_probs, o.log_probs, sizeof(float) * nb, hipMemcpyDeviceToHost, s));
    if (o.lengths) HIPCHK(h, hipMemcpyAsync(p.lengths, o.lengths, sizeof(int32_t) * nb, hipMemcpyDeviceToHost, s));
    if (sl.res.moves) {
      const MovesOut &m = sl.res.moves_out, &q = cx->pin_moves;
      const void* src[6] = {m.raw_pos, m.raw_mass, m.event_pos, m.event_mass, m.peak, m.peak_weight};
      void* dst[6] = {q.raw_pos, q.raw_mass, q.event_pos, q.event_mass, q.peak, q.peak_weight};
      for (int i = 0; i < 6; ++i) if (src[i]) HIPCHK(h, hipMemcpyAsync(dst[i], src[i], 4 * n, hipMemcpyDeviceToHost, s));
    }
  } else if (!dev_out && !calls) {
    HIPCHK(h, hipMemcpyAsync(cx->pin_tok, sl.call.tokens, sizeof(int32_t) * B * steps, hipMemcpyDeviceToHost, s));
    HIPCHK(h, hipMemcpyAsync(cx->pin_out2, sl.call.out2, sizeof(float) * B * steps * (greedy ? V : 1), hipMemcpyDeviceToHost, s));
  }
  if (sl.call.stitch) {      // a stitch slab: the calls and their positions stay on the device, in the rows of the caller's stitch buffer
    const RvStitchBuf* sb = sl.call.stitch;
    const size_t r0 = (size_t)sl.call.stitch_row0, at = r0 * steps, n = (size_t)B * steps;
    const MovesOut& m = sl.res.moves_out;
    const float* src[4] = {m.raw_pos, m.raw_mass, m.event_pos, m.event_mass};
    for (int i = 0; i < 4; ++i) HIPCHK(h, hipMemcpyAsync(sb->mv[i] + at, src[i], sizeof(float) * n, hipMemcpyDeviceToDevice, s));
    HIPCHK(h, hipMemcpyAsync(sb->bases + at, cx->d_bases, n, hipMemcpyDeviceToDevice, s));
    HIPCHK(h, hipMemcpyAsync(sb->probs + at, cx->d_probs, sizeof(float) * n, hipMemcpyDeviceToDevice, s));
    HIPCHK(h, hipMemcpyAsync(sb->lens + r0, cx->d_clen, sizeof(int) * B, hipMemcpyDeviceToDevice, s));
    return RV_OK;
  }
  if (sl.res.call_moves || (sl.res.forced_moves && !dev_out)) {
    const MovesOut &m = sl.res.moves_out, &q = cx->pin_moves;
    const void* src[6] = {m.raw_pos, m.raw_mass, m.event_pos, m.event_mass, m.peak, m.peak_weight};
    void* dst[6] = {q.raw_pos, q.raw_mass, q.event_pos, q.event_mass, q.peak, q.peak_weight};
    for (int i = 0; i < 6; ++i) if (src[i]) HIPCHK(h, hipMemcpyAsync(dst[i], src[i], 4 * (size_t)B * steps, hipMemcpyDeviceToHost, s));
  }
  if (calls) {
    HIPCHK(h, hipMemcpyAsync(cx->pin_bases, cx->d_bases, (size_t)B * steps, hipMemcpyDeviceToHost, s));
    HIPCHK(h, hipMemcpyAsync(cx->pin_probs, cx->d_probs, sizeof(float) * B * steps, hipMemcpyDeviceToHost, s));
    HIPCHK(h, hipMemcpyAsync(cx->pin_clen, cx->d_clen, sizeof(int) * B, hipMemcpyDeviceToHost, s));
  }
  return RV_OK;
}

// The stream work of one slab, in order: input copies, encoders, memory set-up, decode, finalize, output copies.  `ptab` non-null =
// the call is being captured into a slab graph: kernels that touch caller memory read its address from the table.
int record_slab(SlabCtx* cx, const Call& call, const CallParts& res, const Plan& plan, const void* const* ptab) {
  Slab sl{call, res, plan, ptab, call.T_r + call.T_e, call.L - 1};
  TRY(stage_inputs(cx, sl));
  TRY(record_encoders(cx, sl));
  TRY(record_keys(cx, sl));
  TRY(fill_dec_state(cx, sl));
  TRY(split_decode(cx, sl));
  TRY(plan.persist >= 0 ? decode_persist(cx, sl) : decode_steps(cx, sl));
  TRY(finalize_and_score(cx, sl));
  TRY(stage_outputs(cx, sl));
  cx->fact.lW = sl.d.W;
  return RV_OK;
}

// The rest of a call: wait for the context's stream, hand the staged results to the caller's host buffers.
int finish(SlabCtx* cx, int32_t* tokens, float* out2, const CallsOut* calls, int32_t* S_out, const RvBeams* beams = nullptr,
           const RvMoves* moves = nullptr, const RvCallMoves* cmoves = nullptr, bool stitch = false) {
  RvContext* const h = cx->h;
  if (!S_out) return RV_EINVAL;
  if (!cx->pend.busy) return fail(h, RV_ESTATE, "no call to collect on this context");
  const SlabCtx::PendingCall p = cx->pend;
  *S_out = 0;
  if (p.stitch != stitch)      // (the ticket stays in flight)
    return fail(h, RV_EINVAL, p.stitch ? "this call's results went to a stitch buffer: collect it with rv_beam_search_collect_stitch"
                                       : "rv_beam_search_collect_stitch takes the tickets of rv_beam_search_submit_windows_stitch");
  if (p.stitch) {              // nothing to hand out: the slab's copies into the stitch buffer are behind its stream
    cx->pend.busy = false;
    if (p.trivial) return RV_OK;
    HIPCHK(h, hipSetDevice(h->cfg.device));
    HIPCHK(h, hipStreamSynchronize(cx->stream));
    HIPCHK(h, hipGetLastError());
    drain_profile(cx);
    *S_out = *cx->pin_S;
    if (cx->own()) h->lS = *S_out;
    return RV_OK;
  }
  if (p.all != (beams != nullptr) && !(p.all && p.dev_out))      // (the ticket stays in flight)
    return fail(h, RV_EINVAL, p.all ? "this call hands out the whole beam: collect it with rv_beam_search_collect_all"
                                    : "rv_beam_search_collect_all takes the tickets of rv_beam_search_submit_all");
  if (p.moves != (moves != nullptr) && !(p.moves && p.dev_out))      // (the ticket stays in flight)
    return fail(h, RV_EINVAL, p.moves ? "this call hands out the moves: collect it with rv_beam_search_collect_moves"
                                      : "rv_beam_search_collect_moves takes the tickets of rv_beam_search_submit_moves");
  if (p.cmoves != (cmoves != nullptr))      // (the ticket stays in flight)
    return fail(h, RV_EINVAL, p.cmoves ? "this call hands out the positions of its calls: collect it with rv_beam_search_collect_calls_moves"
                                       : "rv_beam_search_collect_calls_moves takes the tickets of rv_beam_search_submit_windows_calls_moves");
  if (p.cmoves && !p.trivial && !cmoves->raw_pos && !cmoves->raw_mass && !cmoves->event_pos && !cmoves->event_mass && !cmoves->peak && !cmoves->peak_weight)
    return fail(h, RV_EINVAL, "null output pointer");
  if (p.moves && !p.dev_out && !p.trivial && !moves->raw_pos && !moves->raw_mass && !moves->event_pos && !moves->event_mass && !moves->peak && !moves->peak_weight)
    return fail(h, RV_EINVAL, "null output pointer");
  cx->pend.busy = false;
  if (p.trivial) {
    if (p.all && !p.dev_out && beams) {      // the initial state
      for (size_t i = 0; i < (size_t)p.B * p.Wd; ++i) {
        if (beams->log_probs) beams->log_probs[i] = i % p.Wd == 0 ? 0.f : -INFINITY;
        if (beams->lengths) beams->lengths[i] = 0;
      }
    }
    return RV_OK;
  }
  if (p.all && !p.dev_out && (!beams->tokens || !beams->scores)) return fail(h, RV_EINVAL, "null output pointer");
  if (!p.all && !p.dev_out && !p.calls && (!tokens || !out2)) return fail(h, RV_EINVAL, "null output pointer");
  if (p.calls && (!calls || !calls->bases || !calls->lengths || !calls->probs)) return fail(h, RV_EINVAL, "null calls output pointer");
  HIPCHK(h, hipSetDevice(h->cfg.device));
  HIPCHK(h, hipStreamSynchronize(cx->stream));
  HIPCHK(h, hipGetLastError());
  const int S = *cx->pin_S;
  const size_t B = p.B, steps = p.steps;
  if (p.all && !p.dev_out) {
    const BeamsOut& q = cx->pin_beams;
    const size_t n = B * steps * p.Wd, nb = B * p.Wd;
    memcpy(beams->tokens, q.tokens, sizeof(int32_t) * n);
    memcpy(beams->scores, q.scores, sizeof(float) * n);
    if (beams->path_scores) memcpy(beams->path_scores, q.path_scores, sizeof(float) * n);
    if (beams->log_probs) memcpy(beams->log_probs, q.log_probs, sizeof(float) * nb);
    if (beams->lengths) memcpy(beams->lengths, q.lengths, sizeof(int32_t) * nb);
    if (p.moves) {
      const MovesOut& m = cx->pin_moves;
      const void* src[6] = {m.raw_pos, m.raw_mass, m.event_pos, m.event_mass, m.peak, m.peak_weight};
      void* dst[6] = {moves->raw_pos, moves->raw_mass, moves->event_pos, moves->event_mass, moves->peak, moves->peak_weight};
      for (int i = 0; i < 6; ++i) if (dst[i]) memcpy(dst[i], src[i], 4 * n);
    }
  } else if (!p.dev_out && !p.calls) {
    memcpy(tokens, cx->pin_tok, sizeof(int32_t) * B * steps);
    memcpy(out2, cx->pin_out2, sizeof(float) * B * steps * (p.greedy ? p.V : 1));
  }
  if (p.calls) {
    memcpy(calls->bases, cx->pin_bases, B * steps);
    memcpy(calls->probs, cx->pin_probs, sizeof(float) * B * steps);
    memcpy(calls->lengths, cx->pin_clen, sizeof(int) * B);
  }
  if (p.cmoves) {
    const MovesOut& m = cx->pin_moves;
    const void* src[6] = {m.raw_pos, m.raw_mass, m.event_pos, m.event_mass, m.peak, m.peak_weight};
    void* dst[6] = {cmoves->raw_pos, cmoves->raw_mass, cmoves->event_pos, cmoves->event_mass, cmoves->peak, cmoves->peak_weight};
    for (int i = 0; i < 6; ++i) if (dst[i]) memcpy(dst[i], src[i], 4 * B * steps);
  }
  drain_profile(cx);
  *S_out = S;
  if (cx->own()) h->lS = S;
  return RV_OK;
}

int flush_open_group(RvContext* h);
int uncollected(const RvContext* h);

// The whole beam's device buffers and pinned staging of a context, for the host variants of rv_beam_search_all*
int ensure_beam_buffers(SlabCtx* cx) {
  RvContext* const h = cx->h;
  if (cx->pin_beams.tokens) return RV_OK;
  const RvConfig& c = h->cfg;
  const size_t n = (size_t)cx->cap * c.max_output_len * c.max_beam, nb = (size_t)cx->cap * c.max_beam;
  HIPCHK(h, hipSetDevice(c.device));
  BeamsOut& d = cx->d_beams;
  BeamsOut& p = cx->pin_beams;
  TRY(dalloc(cx, &d.tokens, n)); TRY(dalloc(cx, &d.scores, n)); TRY(dalloc(cx, &d.path_scores, n));
  TRY(dalloc(cx, &d.log_probs, nb)); TRY(dalloc(cx, &d.lengths, nb));
  HIPCHK(h, hipHostMalloc((void**)&p.scores, n * sizeof(float), hipHostMallocDefault));
  HIPCHK(h, hipHostMalloc((void**)&p.path_scores, n * sizeof(float), hipHostMallocDefault));
  HIPCHK(h, hipHostMalloc((void**)&p.log_probs, nb * sizeof(float), hipHostMallocDefault));
  HIPCHK(h, hipHostMalloc((void**)&p.lengths, nb * sizeof(int32_t), hipHostMallocDefault));
  HIPCHK(h, hipHostMalloc((void**)&p.tokens, n * sizeof(int32_t), hipHostMallocDefault));      // (last: its address says the set is complete)
  return RV_OK;
}

// Before enqueue() of an all-beams call on `ctx`: where its finalize kernel writes.  call.beams null = every output, to the context's
// own buffers (an asynchronous call with host outputs: what is asked for is known at its collect); dev_out = the caller's addresses
int begin_all_beams(SlabCtx* ctx, const Call& call, CallParts& res) {
  const RvBeams* ab = call.beams;
  if (call.dev_out) {
    res.beams = BeamsOut{ab->tokens, ab->scores, ab->path_scores, ab->log_probs, ab->lengths};
  } else {
    TRY(ensure_beam_buffers(ctx));
    res.beams = ctx->d_beams;
    if (ab && !ab->path_scores) res.beams.path_scores = nullptr;
    if (ab && !ab->log_probs) res.beams.log_probs = nullptr;
    if (ab && !ab->lengths) res.beams.lengths = nullptr;
  }
  res.whole_beam = true;
  return RV_OK;
}

// The records of a moves call and, for the host variants, its six device outputs and their pinned staging
int ensure_moves_buffers(SlabCtx* cx, bool host_outputs) {
  RvContext* const h = cx->h; const RvConfig& c = h->cfg;
  HIPCHK(h, hipSetDevice(c.device));
  if (!cx->d_step_moves) TRY(dalloc(cx, &cx->d_step_moves, (size_t)std::max(c.max_output_len - 1, 1) * cx->cap * c.max_beam * RV_MOVE_COLS));
  if (!host_outputs) return RV_OK;
  const size_t n = (size_t)cx->cap * c.max_output_len * c.max_beam;
  MovesOut& d = cx->d_moves;
  MovesOut& p = cx->pin_moves;
  // each buffer on its own test: a call that failed part-way leaves what it got, and the next one allocates only the rest
  if (!d.raw_pos) TRY(dalloc(cx, &d.raw_pos, n));
  if (!d.raw_mass) TRY(dalloc(cx, &d.raw_mass, n));
  if (!d.event_pos) TRY(dalloc(cx, &d.event_pos, n));
  if (!d.event_mass) TRY(dalloc(cx, &d.event_mass, n));
  if (!d.peak) TRY(dalloc(cx, &d.peak, n));
  if (!d.peak_weight) TRY(dalloc(cx, &d.peak_weight, n));
  void** pins[6] = {(void**)&p.raw_pos, (void**)&p.raw_mass, (void**)&p.event_pos, (void**)&p.event_mass, (void**)&p.peak, (void**)&p.peak_weight};
  for (void** q : pins)
    if (!*q) HIPCHK(h, hipHostMalloc(q, n * 4, hipHostMallocDefault));
  return RV_OK;
}

// Before enqueue() of a moves call on `ctx` (after begin_all_beams): its records, and where k_dec_finalize_moves writes.  call.moves
// null = every output, to the context's own buffers (an asynchronous call: what is asked for is known at its collect)
int begin_moves(SlabCtx* ctx, const Call& call, CallParts& res) {
  const RvMoves* mv = call.moves;
  TRY(ensure_moves_buffers(ctx, !call.dev_out));
  if (call.dev_out) {
    res.moves_out = MovesOut{mv->raw_pos, mv->raw_mass, mv->event_pos, mv->event_mass, mv->peak, mv->peak_weight};
  } else {
    res.moves_out = ctx->d_moves;
    if (mv && !mv->raw_pos) res.moves_out.raw_pos = nullptr;
    if (mv && !mv->raw_mass) res.moves_out.raw_mass = nullptr;
    if (mv && !mv->event_pos) res.moves_out.event_pos = nullptr;
    if (mv && !mv->event_mass) res.moves_out.event_mass = nullptr;
    if (mv && !mv->peak) res.moves_out.peak = nullptr;
    if (mv && !mv->peak_weight) res.moves_out.peak_weight = nullptr;
  }
  res.moves = true;
  return RV_OK;
}

// Before enqueue() of a calls-with-positions call on `ctx`: its records, and where k_dec_finalize_calls_moves writes -- always the
// context's own buffers (host outputs).  call.call_moves null = every output (an asynchronous call: what is asked for is known at its collect)
int begin_call_moves(SlabCtx* ctx, const Call& call, CallParts& res) {
  const RvCallMoves* mv = call.call_moves;
  TRY(ensure_moves_buffers(ctx, true));
  res.moves_out = ctx->d_moves;
  if (mv && !mv->raw_pos) res.moves_out.raw_pos = nullptr;
  if (mv && !mv->raw_mass) res.moves_out.raw_mass = nullptr;
  if (mv && !mv->event_pos) res.moves_out.event_pos = nullptr;
  if (mv && !mv->event_mass) res.moves_out.event_mass = nullptr;
  if (mv && !mv->peak) res.moves_out.peak = nullptr;
  if (mv && !mv->peak_weight) res.moves_out.peak_weight = nullptr;
  res.call_moves = true;
  return RV_OK;
}

// Before enqueue() of a forced decode with moves (after begin_forced): its records, and where k_forced_moves writes
int begin_forced_moves(SlabCtx* ctx, const Call& call, CallParts& res) {
  const RvMoves* mv = call.forced_moves;
  TRY(ensure_moves_buffers(ctx, !call.dev_out));
  if (call.dev_out) {
    res.moves_out = MovesOut{mv->raw_pos, mv->raw_mass, mv->event_pos, mv->event_mass, mv->peak, mv->peak_weight};
  } else {
    res.moves_out = ctx->d_moves;
    if (!mv->raw_pos) res.moves_out.raw_pos = nullptr;
    if (!mv->raw_mass) res.moves_out.raw_mass = nullptr;
    if (!mv->event_pos) res.moves_out.event_pos = nullptr;
    if (!mv->event_mass) res.moves_out.event_mass = nullptr;
    if (!mv->peak) res.moves_out.peak = nullptr;
    if (!mv->peak_weight) res.moves_out.peak_weight = nullptr;
  }
  res.forced_moves = true;
  return RV_OK;
}

// Labels and score outputs of a context on the device, for the host variants of rv_teacher_forced and for rv_score_logits
int ensure_score_buffers(SlabCtx* cx) {
  RvContext* const h = cx->h;
  if (cx->d_sc_cnt) return RV_OK;
  const RvConfig& c = h->cfg;
  const size_t n = (size_t)cx->cap * c.max_output_len, nb = (size_t)cx->cap;
  HIPCHK(h, hipSetDevice(c.device));
  TRY(dalloc(cx, &cx->d_forced, n)); TRY(dalloc(cx, &cx->d_sc_nll, n)); TRY(dalloc(cx, &cx->d_sc_sum, nb));
  TRY(dalloc(cx, &cx->d_sc_cnt, 3 * nb));      // (last: its address says the set is complete)
  return RV_OK;
}

// Where a call's k_score_tokens writes: the caller's device addresses, or the context's buffers for the outputs a host caller asked for
ScoreArgs score_outputs(const SlabCtx* ctx, const ForcedCall* fc, bool dev_out) {
  const RvScore none{};
  const RvScore& o = fc->out ? *fc->out : none;
  const size_t nb = (size_t)ctx->cap;
  ScoreArgs a{};
  a.omit_mask = fc->omit_mask;
  a.nll = dev_out ? o.nll : (o.nll ? ctx->d_sc_nll : nullptr);
  a.nll_sum = dev_out ? o.nll_sum : (o.nll_sum ? ctx->d_sc_sum : nullptr);
  a.n_labels = dev_out ? o.n_labels : (o.n_labels ? ctx->d_sc_cnt : nullptr);
  a.n_match = dev_out ? o.n_match : (o.n_match ? ctx->d_sc_cnt + nb : nullptr);
  a.n_counted = dev_out ? o.n_counted : (o.n_counted ? ctx->d_sc_cnt + 2 * nb : nullptr);
  return a;
}

// ids [n] all inside [0, vocab)?  (host labels: an id never reaches a kernel unchecked)
int check_token_ids(RvContext* h, const int32_t* ids, size_t n, int row_len, const char* what) {
  const int V = h->cfg.vocab;
  for (size_t i = 0; i < n; ++i)
    if (ids[i] < 0 || ids[i] >= V)
      return fail(h, RV_EINVAL, "%s id %d at [%zu,%zu] outside [0,%d)", what, (int)ids[i], i / row_len, i % row_len, V);
  return RV_OK;
}

// Before enqueue() of a forced decode on the idle context `ctx`: the call's own checks, then its labels and score outputs
int begin_forced(SlabCtx* ctx, const Call& call, CallParts& res) {
  const ForcedCall* fc = call.forced;
  const int B = call.B, L = call.L;
  const bool dev = call.dev_in;      // (a forced decode's buffers are all the host's or all the device's)
  Call one = call, ok;
  one.W = 1;
  TRY(validate_call(ctx, one, ok));
  if (B > 0 && !fc->targets) return fail(ctx->h, RV_EINVAL, "null target pointer");
  if (dev) {
    res.labels = fc->targets;
  } else {
    TRY(check_token_ids(ctx->h, fc->targets, (size_t)B * L, L, "target"));
    TRY(ensure_score_buffers(ctx));
    if (B > 0) HIPCHK(ctx->h, hipMemcpy(ctx->d_forced, fc->targets, sizeof(int32_t) * (size_t)B * L, hipMemcpyHostToDevice));
    res.labels = ctx->d_forced;
  }
  res.score = score_outputs(ctx, fc, dev);
  return RV_OK;
}

// After the stream of the call's context has drained: the scores of B chunks x S positions (k_score_tokens wrote them through `a`) to a host
// caller's buffers (zeros when nothing was launched)
int fetch_scores(RvContext* h, const ScoreArgs& a, const RvScore* out, bool dev_out, int B, int S) {
  if (!out || B <= 0) return RV_OK;
  const size_t nb = (size_t)B, n = nb * (size_t)std::max(S, 0);
  if (S <= 0) {      // nothing ran: every per-chunk sum is zero
    if (dev_out) {
      if (out->nll_sum) HIPCHK(h, hipMemset(out->nll_sum, 0, sizeof(float) * nb));
      for (int32_t* p : {out->n_labels, out->n_match, out->n_counted}) if (p) HIPCHK(h, hipMemset(p, 0, sizeof(int32_t) * nb));
    } else {
      if (out->nll_sum) memset(out->nll_sum, 0, sizeof(float) * nb);
      for (int32_t* p : {out->n_labels, out->n_match, out->n_counted}) if (p) memset(p, 0, sizeof(int32_t) * nb);
    }
    return RV_OK;
  }
  if (dev_out) return RV_OK;
  if (out->nll) HIPCHK(h, hipMemcpy(out->nll, a.nll, sizeof(float) * n, hipMemcpyDeviceToHost));
  if (out->nll_sum) HIPCHK(h, hipMemcpy(out->nll_sum, a.nll_sum, sizeof(float) * nb, hipMemcpyDeviceToHost));
  if (out->n_labels) HIPCHK(h, hipMemcpy(out->n_labels, a.n_labels, sizeof(int32_t) * nb, hipMemcpyDeviceToHost));
  if (out->n_match) HIPCHK(h, hipMemcpy(out->n_match, a.n_match, sizeof(int32_t) * nb, hipMemcpyDeviceToHost));
  if (out->n_counted) HIPCHK(h, hipMemcpy(out->n_counted, a.n_counted, sizeof(int32_t) * nb, hipMemcpyDeviceToHost));
  return RV_OK;
}

// The slab context a synchronous call runs on.  A group of coalesced slabs that is still filling is launched first.
int sync_context(RvContext* h, SlabCtx** out) {
  {   // coalesced tickets hold the handle's slots as the slab contexts' tickets do: with async_depth of them uncollected a synchronous
      // call is refused, touching nothing (slot 0 is idle then, but the contract does not depend on the path)
    bool ticks_out = false;
    for (const auto& t : h->ticks) ticks_out = ticks_out || t.busy;
    if (ticks_out && uncollected(h) >= async_depth(h))
      return fail(h, RV_ESTATE, "every slab context of this handle holds an uncollected asynchronous call: collect one before a synchronous call");
  }
  flush_open_group(h);      // (a group still filling goes first; a failure there is its tickets')
  // A synchronous call between asynchronous ones: it runs on slot 0 when that one is idle, else on any idle context of the handle --
  // never on one that still holds an uncollected ticket (its stream work and output pointers are live).  Debug taps and rv_get_tensor
  // belong to slot 0 (SlabCtx::own), so with taps on that context must be the idle one.
  SlabCtx* ctx = nullptr;
  for (SlabCtx* k : h->slabs) if (!k->pend.busy) { ctx = k; break; }      // (slot 0 first)
  if (h->slabs[0]->pend.busy && (h->opt.taps || h->opt.ptaps))
    return fail(h, RV_ESTATE, "debug taps need the handle's own context, which holds an uncollected asynchronous call: collect ticket %d first", h->slabs[0]->pend.ticket);
  if (!ctx) return fail(h, RV_ESTATE, "every slab context of this handle holds an uncollected asynchronous call: collect one before a synchronous call");
  h->inflight_hint = 1;
  *out = ctx;
  return RV_OK;
}

// A synchronous call: what a kind of call adds to the plain one is resolved into `res`, which lives in this frame until the call is done
int run(RvContext* h, const Call& call, int32_t* S_out) {
  if (!h) return RV_EINVAL;
  const CallsOut* calls = call.calls;
  if (!S_out || (call.B > 0 && call.L > 1 && !calls && (!call.tokens || !call.out2))) return fail(h, RV_EINVAL, "null output pointer");
  if (calls && (!calls->lut || !calls->bases || !calls->lengths || !calls->probs)) return fail(h, RV_EINVAL, "null calls output pointer");
  *S_out = 0;
  SlabCtx* ctx = nullptr;
  TRY(sync_context(h, &ctx));
  CallParts res;
  if (call.whole_beam) TRY(begin_all_beams(ctx, call, res));
  if (call.want_moves) TRY(begin_moves(ctx, call, res));
  if (call.want_call_moves) TRY(begin_call_moves(ctx, call, res));
  if (call.forced) TRY(begin_forced(ctx, call, res));
  if (call.forced_moves) TRY(begin_forced_moves(ctx, call, res));
  const int rc = enqueue(ctx, call, res);
  if (rc != RV_OK) { ctx->pend.busy = false; return rc; }   // (ctx was idle on entry: the flag is this call's)
  int rf = finish(ctx, call.tokens, call.out2, calls, S_out, call.beams, call.moves, call.call_moves);
  if (call.forced && rf == RV_OK) rf = fetch_scores(h, res.score, call.forced->out, call.dev_out, call.B, call.L - 1);
  if (call.forced_moves && rf == RV_OK && !call.dev_out && call.B > 0 && call.L > 1) {      // staged by stage_outputs; the stream has drained
    const MovesOut& m = ctx->pin_moves;
    const RvMoves* o = call.forced_moves;
    const void* src[6] = {m.raw_pos, m.raw_mass, m.event_pos, m.event_mass, m.peak, m.peak_weight};
    void* dst[6] = {o->raw_pos, o->raw_mass, o->event_pos, o->event_mass, o->peak, o->peak_weight};
    for (int i = 0; i < 6; ++i) if (dst[i]) memcpy(dst[i], src[i], 4 * (size_t)call.B * (call.L - 1));
  }
  h->lS = *S_out;      // (whichever slot it ran on: finish() leaves the two equal on slot 0)
  return rf;
}

// Per-slab working set of a context, for cx->cap chunks: inputs, activations, decoder state, outputs, staging, side streams
int alloc_slab_buffers(SlabCtx* cx) {
  RvContext* const h = cx->h; const RvConfig& c = h->cfg;
  const bool use_raw = c.mode != RV_MODE_EVENT, use_ev = c.mode != RV_MODE_RAW;
  const size_t B = cx->cap, Tr = use_raw ? c.max_raw_len : 0, Te = use_ev ? c.max_event_len : 0;
  const size_t Tm = Tr + Te, L = c.max_output_len, N = B * c.max_beam, V = c.vocab;
  TRY(dalloc(cx, &cx->d_raw, B * Tr));
  TRY(dalloc(cx, &cx->d_ev, B * Te * 5));
  TRY(dalloc(cx, &cx->mask, B * Tm));
  const int npp = c.enc_depth > 2 ? 2 : (c.enc_depth > 1 ? 1 : 0);
  for (int p = 0; p < npp; ++p) {
    if (use_raw) TRY(dalloc(cx, &cx->act[0][p], B * Tr * RV_E));
    if (use_ev) TRY(dalloc(cx, &cx->act[1][p], B * Te * RV_E));
  }
  // The pre-projected tensors xw [max_batch, T_max, 2, 512] (4 KB per chunk-timestep) of the matrix-pipe recurrence (the default) and of the
  // unfused packed-FMA path: allocated HERE, with the context -- not on a context's first call.  (Round 4 found the first-use hipMalloc of a
  // fresh context inside bench.py's timed region: the driver's 5 warm-up steps touch 5 of the 10 contexts, the other five allocated 2 x ~300 MB
  // each while the GPU drained -- 1.5 to 10 ms of host stall per context, which rounds 3 and 4 had read as the pipeline's fill time.)
  if (use_raw && c.enc_depth > 1) TRY(dalloc(cx, &cx->xw[0], B * Tr * 2 * RV_G));
  if (use_ev) TRY(dalloc(cx, &cx->xw[1], B * Te * 2 * RV_G));
  for (int e = 0; e < 2; ++e)
    for (int st = 0; st < 2; ++st)
      for (int k = 0; k < 4; k += h->rnn == RV_RNN_BIGRU ? 2 : 1) TRY(dalloc(cx, &cx->st[e][st][k], B * RV_U));      // (a GRU's sets hold h only)
  TRY(dalloc(cx, &cx->enc_out, B * Tm * RV_E));
  TRY(dalloc(cx, &cx->keys, B * Tm * RV_U));
  if (h->rnn == RV_RNN_BILSTM || h->gimg.allocated) TRY(dalloc(cx, &cx->mem2, B * Tm * RV_E));      // (the persistent decode's projected memory; a GRU handle: under option gru_persistent)
  DecState& d = cx->dec_st;
#ifdef RV_DIAG   // timing ablations that INVALIDATE results: only in `make diag` builds (libravvent_hip_diag.so), never in the product library
  if (const char* e = getenv("RV_ATT_STOP")) d.dbg_stop = atoi(e);
#endif
  if (getenv("RV_REC_STAMPS")) { TRY(dalloc(cx, &cx->rec_ts, 24)); cx->rec_ts_layer = atoi(getenv("RV_REC_STAMPS")) == 2 ? 1 : 0; }
  if (getenv("RV_DBG_STAMPS")) TRY(dalloc(cx, &d.dbg_ts, 16));   // diagnostic builds: in-kernel phase stamps   // timing ablation only; results are invalid when set
  d.depth = c.dec_depth; d.ls_xh = N * RV_E; d.ls_c = N * RV_U;
  TRY(dalloc(cx, &d.xh, c.dec_depth * N * RV_E));
  TRY(dalloc(cx, &d.z, N * RV_G));
  TRY(dalloc(cx, &d.c, c.dec_depth * N * RV_U));
  TRY(dalloc(cx, &d.c_new, c.dec_depth * N * RV_U));
  TRY(dalloc(cx, &d.h_new, c.dec_depth * N * RV_U));
  TRY(dalloc(cx, &d.tok, N));
  TRY(dalloc(cx, &d.log_probs, N));
  TRY(dalloc(cx, &d.finished, N));
  TRY(dalloc(cx, &d.lengths, N));
  TRY(dalloc(cx, &d.step_ids, L * N));
  TRY(dalloc(cx, &d.parent_ids, L * N));
  TRY(dalloc(cx, &d.step_scores, L * N));
  TRY(dalloc(cx, &d.step_logits, L * N * V));
  TRY(dalloc(cx, &d.nfin, 4 * (L + 1)));
  TRY(dalloc(cx, &d.S_dev, 8));
  TRY(dalloc(cx, &cx->d_chunk_steps, B));
  // (side streams are created on first use -- side_stream(): the contexts of the asynchronous calls never need them, and every
  //  stream of the process competes for the same few hardware queues)
  for (int g = 0; g < 3; ++g) HIPTRY(hipEventCreateWithFlags(&cx->ev_join[g], hipEventDisableTiming));
  HIPTRY(hipEventCreateWithFlags(&cx->ev_fork, hipEventDisableTiming));
  TRY(dalloc(cx, &cx->out_tokens, B * L));
  TRY(dalloc(cx, &cx->out2, B * L * V));
  HIPTRY(hipHostMalloc((void**)&cx->pin_raw, std::max<size_t>(B * Tr, 1) * sizeof(float), hipHostMallocDefault));
  HIPTRY(hipHostMalloc((void**)&cx->pin_ev, std::max<size_t>(B * Te * 5, 1) * sizeof(float), hipHostMallocDefault));
  HIPTRY(hipHostMalloc((void**)&cx->pin_tok, B * L * sizeof(int32_t), hipHostMallocDefault));
  HIPTRY(hipHostMalloc((void**)&cx->pin_out2, B * L * V * sizeof(float), hipHostMallocDefault));
  HIPTRY(hipHostMalloc((void**)&cx->pin_S, sizeof(int) * RV_MAX_MEMBERS, hipHostMallocMapped));
  HIPTRY(hipHostGetDevicePointer((void**)&d.S_host, cx->pin_S, 0));
  TRY(dalloc(cx, &cx->d_bases, B * L));
  TRY(dalloc(cx, &cx->d_probs, B * L));
  TRY(dalloc(cx, &cx->d_clen, B));
  HIPTRY(hipHostMalloc((void**)&cx->pin_bases, B * L, hipHostMallocDefault));
  HIPTRY(hipHostMalloc((void**)&cx->pin_probs, B * L * sizeof(float), hipHostMallocDefault));
  HIPTRY(hipHostMalloc((void**)&cx->pin_clen, B * sizeof(int), hipHostMallocDefault));
  // the table lives in mapped pinned memory: the three kernels that need a caller address read it over the host link once per workgroup
  // (a device copy refreshed by a memcpy node in front of the graph measured the same, and is one node more)
  TRY(dalloc(cx, &cx->d_win, B));
  HIPTRY(hipHostMalloc((void**)&cx->pin_win, std::max<size_t>(B, 1) * sizeof(RecWindow), hipHostMallocDefault));
  HIPTRY(hipHostMalloc((void**)&cx->pin_ptab, sizeof(void*) * RV_PTAB_N, hipHostMallocMapped));
  HIPTRY(hipHostGetDevicePointer((void**)&cx->d_ptab, cx->pin_ptab, 0));
  return RV_OK;
}

// Everything a slab context owns; its stream drains first
void destroy_slab(SlabCtx* cx) {
  if (!cx) return;
  if (cx->stream) hipStreamSynchronize(cx->stream);
  for (auto& kv : cx->graphs) hipGraphExecDestroy(kv.second);
  for (auto& kv : cx->slab_graphs) hipGraphExecDestroy(kv.second.exec);
  for (auto& p : cx->pending) { hipEventDestroy(p.a); hipEventDestroy(p.b); }
  for (auto e : cx->ev_pool) hipEventDestroy(e);
  for (int g = 0; g < 3; ++g) { if (cx->side[g]) hipStreamDestroy(cx->side[g]); if (cx->ev_join[g]) hipEventDestroy(cx->ev_join[g]); }
  if (cx->ev_fork) hipEventDestroy(cx->ev_fork);
  if (cx->step_align) hipFree(cx->step_align);
  if (cx->palign) hipFree(cx->palign);
  for (void* p : {(void*)cx->pin_raw, (void*)cx->pin_ev, (void*)cx->pin_tok, (void*)cx->pin_out2, (void*)cx->pin_S, (void*)cx->pin_bases, (void*)cx->pin_probs, (void*)cx->pin_clen, (void*)cx->pin_ptab, (void*)cx->pin_win,
                  (void*)cx->pin_beams.tokens, (void*)cx->pin_beams.scores, (void*)cx->pin_beams.path_scores, (void*)cx->pin_beams.log_probs, (void*)cx->pin_beams.lengths,
                  (void*)cx->pin_moves.raw_pos, (void*)cx->pin_moves.raw_mass, (void*)cx->pin_moves.event_pos, (void*)cx->pin_moves.event_mass, (void*)cx->pin_moves.peak, (void*)cx->pin_moves.peak_weight}) if (p) hipHostFree(p);
  for (void* p : cx->allocs) hipFree(p);
  if (cx->stream) hipStreamDestroy(cx->stream);
  delete cx;
}

// A slab context of handle h for `cap` chunks: own stream and buffers.  slot: its place in h->slabs, -1 for a group's context
int create_slab(RvContext* h, SlabCtx** out, int cap, int slot) {
  SlabCtx* cx = new SlabCtx();
  cx->h = h; cx->cap = cap; cx->slot = slot;
  // (stream priorities -- the contexts at the runtime's three levels in turn, so that slabs submitted together leave lockstep -- measured
  //  no gain at the driver's 20 steps and 4 % less once the stream has settled: tools/stream_ab.py, round 4)
  if (hipStreamCreateWithFlags(&cx->stream, hipStreamNonBlocking) != hipSuccess) {
    delete cx;
    return fail(h, RV_EHIP, slot == 0 ? "hipStreamCreate failed" : "hipStreamCreate failed for an asynchronous context");
  }
  const int rc = alloc_slab_buffers(cx);
  if (rc != RV_OK) { destroy_slab(cx); return rc; }
  *out = cx;
  return RV_OK;
}

void destroy_group(Group* g) {      // (launched or still filling: its stream drains in there)
  destroy_slab(g->ctx);
  delete g;
}

// ---- coalesced asynchronous calls
int hw_queues(const char** text = nullptr) {       // what the runtime was (or will be) started with (*text: as the environment words it, null = unset)
  const char* q = getenv("GPU_MAX_HW_QUEUES");
  if (text) *text = q;
  const int nq = q ? atoi(q) : 4;
  return nq > 0 ? nq : 4;
}

// Slabs per group.  An explicit option value holds (up to the depth and the member table).  The default never holds back the slab of a
// caller that submits one and then works on the CPU (depth <= 3), never exceeds depth / 2 (one group runs while the next fills), and
// coalesces only where the contexts outnumber the hardware queues -- with a queue per context the slabs overlap by themselves
// (profiles/coalesce.md has the sweep behind the numbers).
int coalesce_n(const RvContext* h, int depth) {
  if (h->opt.coalesce >= 0) return std::max(1, std::min({h->opt.coalesce, depth, RV_MAX_MEMBERS}));
  if (depth <= 3 || hw_queues() >= depth) return 1;
  return depth < 8 ? 2 : std::min(depth / 2, 5);      // (C3 on 4 queues: depth 4 and 6 stream fastest with 2, depth 10 with 5)
}

// Does a group run its event encoder on a side stream beside its raw encoder (record_encoders)?  By default where every group context in
// flight, ceil(depth / n) of them, gets a hardware queue for its own stream and one for its side stream (C3 at the defaults on 4 queues:
// two groups of five; profiles/group_chain.md).
bool group_side_ev(const RvContext* h) {
  if (h->opt.group_side_ev >= 0) return h->opt.group_side_ev != 0;
  const int depth = async_depth(h), n = coalesce_n(h, depth);
  return 2 * ((depth + n - 1) / n) <= hw_queues();
}

int uncollected(const RvContext* h) {
  int n = 0;
  for (const SlabCtx* k : h->slabs) n += k->pend.busy ? 1 : 0;
  for (const auto& t : h->ticks) n += t.busy ? 1 : 0;
  return n;
}

// Does this (validated) slab take the default streamed path, the only one that is coalesced?
bool coalescible(const RvContext* h, const Call& call) {
  const SlabCtx* cx = h->slabs[0];      // (the plan of a plain beam search is the same on every slot once the taps are off)
  if (h->opt.profile != 0 || h->opt.taps || h->opt.ptaps || cx->rec_ts || cx->dec_st.dbg_ts || h->opt.slab_graph || call.L <= 1) return false;
  if (h->rnn != RV_RNN_BILSTM) return false;      // (the group kernels are the BiLSTM's: a GRU handle's slabs run one by one, persistent decode or not)
  const Plan p = plan_call(cx, call, CallParts{});
  return p.wide && p.persist >= 0;
}

void reset_group(Group* g) {
  g->n = 0; g->rows = 0; g->staged = 0; g->launched = false; g->synced = false; g->failed = RV_OK;
}

// Can the layer-0 kernels of a group of this shape read their members' device inputs in place?  Only the matrix-pipe layer 0 with its
// input projection in the lane resolves a chunk to its member (rec_mx_body); coalescible() has settled that for the raw encoder.
bool inplace_serves(const RvContext* h, int T_e) {
  return h->opt.group_inplace && (h->cfg.mode == RV_MODE_RAW || lane_layer0(h, 5, T_e));
}

// Queue a group's internal call: its members' inputs are in d_raw / d_ev already, back to back, or stay where the callers hold them (submit_group).
int launch_group(RvContext* h, Group* g) {
  if (h->open_grp == g) h->open_grp = nullptr;
  if (g->launched) return g->failed;
  g->launched = true;
  h->co_groups += 1; h->co_slabs += g->n; h->co_largest = std::max<long long>(h->co_largest, g->n);
  if (g->rows == 0) return RV_OK;          // empty slabs only: nothing to run, S = 0
  const size_t steps = (size_t)g->L - 1;
  DecMembers& m = g->members;
  m.n = g->n;
  for (int i = 0; i < g->n; ++i) {
    const Tick& t = h->ticks[g->tslot[i]];
    m.row0[i] = t.row0; m.rows[i] = t.B;
    for (RecMembers& in : g->in) { in.n = g->n; in.row0[i] = t.row0; in.rows[i] = t.B; }
    if (!g->dev_out) { m.tokens[i] = g->ctx->out_tokens + (size_t)t.row0 * steps; m.out2[i] = g->ctx->out2 + (size_t)t.row0 * steps; }
  }
  Call call;
  call.raw = g->ctx->d_raw; call.ev = g->ctx->d_ev; call.dev_in = true;
  call.B = g->rows; call.T_r = g->Tr; call.T_e = g->Te; call.W = g->W; call.L = g->L;
  call.tokens = g->ctx->out_tokens; call.out2 = g->ctx->out2; call.dev_out = g->dev_out;
  call.lut = g->calls ? g->lut : nullptr;
  if (g->win) { call.raw = call.ev = nullptr; call.windows = g->ctx->pin_win; }
  CallParts res;
  res.members = &m;
  res.form_B = g->B0;
  const int rc = enqueue(g->ctx, call, res);
  h->gforms = g->ctx->lforms;
  g->ctx->pend.busy = false;                 // (the tickets live in the handle's table)
  if (rc != RV_OK) g->failed = rc;
  return rc;
}

int flush_open_group(RvContext* h) { return h->open_grp ? launch_group(h, h->open_grp) : RV_OK; }

// A (validated, coalescible) slab joins the open group of n slabs, opening one if need be; the group is launched when it is full
int submit_group(RvContext* h, int n, const Call& call, int32_t* ticket) {
  const RvConfig& c = h->cfg;
  const float *raw = call.raw, *ev = call.ev;
  const int B = call.B, T_r = call.T_r, T_e = call.T_e, W = call.W, L = call.L;
  const bool dev_in = call.dev_in, dev_out = call.dev_out;
  const uint8_t* lut = call.lut;
  const bool calls = lut != nullptr;
  const bool win = call.windows != nullptr;
  HIPCHK(h, hipSetDevice(c.device));
  Group* g = h->open_grp;
  if (g && (g->cap != n || g->win != win || g->Tr != T_r || g->Te != T_e || g->W != W || g->L != L || g->dev_in != dev_in || g->dev_out != dev_out ||
            g->calls != calls || (calls && memcmp(g->lut, lut, (size_t)c.vocab)))) {
    launch_group(h, g);                      // another shape or kind: the group goes as it is (a failure is its members' to collect)
    g = nullptr;
  }
  if (!g) {
    for (size_t i = 0; i < h->groups.size() && !g; ++i) {
      Group* cand = h->groups[i];
      if (cand->n != 0) continue;
      if (cand->cap == n) { g = cand; break; }
      destroy_group(cand);                     // idle, sized for another group size (the option changed)
      h->groups.erase(h->groups.begin() + i); --i;
    }
    // the group contexts an in-order stream needs, ceil(depth / n), exist from the first coalesced submit on, as the slab contexts do from the
    // first submit: none is allocated (gigabytes of hipMalloc at C3 sizes) in the middle of a stream.  One more only when none is idle
    const int depth = async_depth(h);
    while (!g || (int)h->groups.size() < (depth + n - 1) / n) {
      SlabCtx* cx = nullptr;
      TRY(create_slab(h, &cx, n * h->cfg.max_batch, -1));      // (room for n slabs back to back)
      Group* k = new Group();
      k->ctx = cx; k->cap = n;
      cx->grp = k;
      if (group_side_ev(h)) side_stream(cx, 0);     // (created with the context, as its buffers are: not at a group's first launch in mid-stream)
      reset_group(k);
      h->groups.push_back(k);
      if (!g) g = k;
    }
    reset_group(g);
    g->Tr = T_r; g->Te = T_e; g->W = W; g->L = L; g->dev_in = dev_in; g->dev_out = dev_out; g->calls = calls; g->B0 = B;
    g->win = win;
    g->inplace = dev_in && !win && inplace_serves(h, T_e);      // (the options cannot change under an open group: rv_set_option launches it)
    memset(g->lut, 0, sizeof g->lut);
    if (calls) memcpy(g->lut, lut, (size_t)c.vocab);
    h->open_grp = g;
  }
  int slot = -1;
  for (int i = 0; i < RV_MAX_ASYNC && slot < 0; ++i) if (!h->ticks[i].busy) slot = i;
  if (slot < 0) return fail(h, RV_ESTATE, "no free ticket");      // (unreachable: at most async_depth <= RV_MAX_ASYNC are uncollected)
  const size_t row0 = (size_t)g->rows;
  if (win) {            // the member's rows behind those of the members before it: the group's table needs no member lookup
    if (B > 0) memcpy(g->ctx->pin_win + row0, call.windows, sizeof(RecWindow) * (size_t)B);
  } else if (g->inplace) {   // device inputs stay valid and untouched until the ticket is collected (ravvent_hip.h): the layer-0 kernels read them there
    g->in[0].x[g->n] = raw; g->in[1].x[g->n] = ev;
  } else if (B > 0) {   // the member's inputs go to its rows of the group's input buffers now: the caller's host buffers are free on return
    const size_t nr = (size_t)B * T_r, ne = (size_t)B * T_e * 5;
    if (!dev_in) {
      if (nr) { memcpy(g->ctx->pin_raw + row0 * T_r, raw, sizeof(float) * nr); HIPCHK(h, hipMemcpyAsync(g->ctx->d_raw + row0 * T_r, g->ctx->pin_raw + row0 * T_r, sizeof(float) * nr, hipMemcpyHostToDevice, g->ctx->stream)); }
      if (ne) { memcpy(g->ctx->pin_ev + row0 * T_e * 5, ev, sizeof(float) * ne); HIPCHK(h, hipMemcpyAsync(g->ctx->d_ev + row0 * T_e * 5, g->ctx->pin_ev + row0 * T_e * 5, sizeof(float) * ne, hipMemcpyHostToDevice, g->ctx->stream)); }
    } else {
      if (nr) HIPCHK(h, hipMemcpyAsync(g->ctx->d_raw + row0 * T_r, raw, sizeof(float) * nr, hipMemcpyDeviceToDevice, g->ctx->stream));
      if (ne) HIPCHK(h, hipMemcpyAsync(g->ctx->d_ev + row0 * T_e * 5, ev, sizeof(float) * ne, hipMemcpyDeviceToDevice, g->ctx->stream));
    }
  }
  const int i = g->n++;
  g->rows += B;
  g->tslot[i] = slot;
  if (dev_out) { g->members.tokens[i] = call.tokens; g->members.out2[i] = call.out2; } else g->staged += 1;
  Tick& t = h->ticks[slot];
  t = Tick{};
  t.busy = true; t.dev_out = dev_out; t.calls = calls; t.member = i; t.B = B; t.row0 = (int)row0; t.steps = L - 1; t.grp = g;
  t.ticket = issue_ticket(h, slot);
  *ticket = t.ticket;
  if (g->n == g->cap) launch_group(h, g);      // (a failed launch is reported when its tickets are collected)
  return RV_OK;
}

int collect_group(RvContext* h, int slot, int32_t* tokens, float* out2, const CallsOut* calls, int32_t* S_out) {
  Tick& t = h->ticks[slot];
  *S_out = 0;
  if (!t.done) {          // the first collect of a group's ticket launches it if need be, waits for it and settles every member's S
    Group* g = t.grp;
    HIPCHK(h, hipSetDevice(h->cfg.device));
    int rc = launch_group(h, g);
    if (rc == RV_OK && g->rows > 0) {
      hipError_t e = hipStreamSynchronize(g->ctx->stream);
      if (e == hipSuccess) e = hipGetLastError();
      if (e != hipSuccess) rc = fail(h, RV_EHIP, "a coalesced call failed: %s", hipGetErrorString(e));
    }
    g->synced = true;
    for (int i = 0; i < g->n; ++i) {
      Tick& u = h->ticks[g->tslot[i]];
      u.done = true; u.S = (rc == RV_OK && u.B > 0) ? g->ctx->pin_S[i] : 0;
      if (rc != RV_OK) u.S = -1;
    }
    if (rc != RV_OK || g->staged == 0) {   // results in the callers' device memory: the context takes the next group now
      for (int i = 0; i < g->n; ++i) h->ticks[g->tslot[i]].grp = nullptr;
      reset_group(g);
    }
  }
  const Tick u = t;
  t.busy = false;
  if (u.S < 0) return fail(h, RV_EHIP, "ticket %d: its coalesced call failed", u.ticket);
  if (u.B > 0 && !u.dev_out) {
    Group* g = u.grp;
    const size_t B = u.B, steps = u.steps, r0 = u.row0;
    int rc = RV_OK;
    if (!u.calls && (!tokens || !out2)) rc = fail(h, RV_EINVAL, "null output pointer");
    else if (u.calls && (!calls || !calls->bases || !calls->lengths || !calls->probs)) rc = fail(h, RV_EINVAL, "null calls output pointer");
    else if (!u.calls) {
      memcpy(tokens, g->ctx->pin_tok + r0 * steps, sizeof(int32_t) * B * steps);
      memcpy(out2, g->ctx->pin_out2 + r0 * steps, sizeof(float) * B * steps);
    } else {
      memcpy(calls->bases, g->ctx->pin_bases + r0 * steps, B * steps);
      memcpy(calls->probs, g->ctx->pin_probs + r0 * steps, sizeof(float) * B * steps);
      memcpy(calls->lengths, g->ctx->pin_clen + r0, sizeof(int) * B);
    }
    if (rc != RV_OK) { if (--g->staged == 0) reset_group(g); return rc; }
  }
  if (!u.dev_out && u.grp && --u.grp->staged == 0) reset_group(u.grp);
  *S_out = u.S;
  h->lS = u.S;
  return RV_OK;
}

// What every entry point states the same way.  An entry point's buffers are all the host's or all the device's (on_device); it adds
// its outputs and what makes its kind of call
Call slab_call(const float* raw, const float* event, bool on_device, int B, int T_r, int T_e, int W, int L) {
  Call c;
  c.raw = raw; c.ev = event; c.dev_in = on_device; c.dev_out = on_device;
  c.B = B; c.T_r = T_r; c.T_e = T_e; c.W = W; c.L = L;
  return c;
}

// ---- reads and window tables (rv_read_put*, rv_beam_search_windows*)
constexpr int RV_READ_SLOTS = 1024;         // read_id = generation << 10 | slot: an id that was dropped is never alive again

Read* find_read(RvContext* h, int id) {
  const int slot = id & (RV_READ_SLOTS - 1);
  if (id < 0 || slot >= (int)h->reads.size()) return nullptr;
  Read& r = h->reads[slot];
  return r.live && r.id == id ? &r : nullptr;
}

// The table of a window call, checked row by row against the reads it names BEFORE anything is queued, so that no kernel ever indexes with
// an unchecked offset: rows [B] as the kernels take them, ids = the reads used (each once).  The columns of the segment the mode does not
// use are ignored (null address, length 0)
int resolve_windows(RvContext* h, const int32_t* win, int B, int T_r, int T_e, std::vector<RecWindow>& rows, std::vector<int>& ids) {
  const RvConfig& c = h->cfg;
  const bool use_raw = c.mode != RV_MODE_EVENT, use_ev = c.mode != RV_MODE_RAW;
  if (B < 0 || B > c.max_batch) return fail(h, RV_EINVAL, "B=%d outside [0,%d]", B, c.max_batch);
  if (B > 0 && !win) return fail(h, RV_EINVAL, "null window table");
  rows.assign((size_t)B, RecWindow{nullptr, nullptr, 0, 0});
  for (int b = 0; b < B; ++b) {
    const int32_t* w = win + (size_t)b * 5;
    const Read* r = find_read(h, w[0]);
    if (!r) return fail(h, RV_EINVAL, "window row %d: unknown read_id %d", b, w[0]);
    if (use_raw) {
      if (w[1] < 0 || w[2] < 0) return fail(h, RV_EINVAL, "window row %d: negative raw start or length (%d, %d)", b, w[1], w[2]);
      if ((long long)w[1] + w[2] > (long long)r->n_raw) return fail(h, RV_EINVAL, "window row %d: raw window [%d, %lld) ends beyond the read's %zu samples", b, w[1], (long long)w[1] + w[2], r->n_raw);
      if (w[2] > T_r) return fail(h, RV_EINVAL, "window row %d: raw_len %d exceeds T_r=%d", b, w[2], T_r);
      rows[b].raw = r->d_raw + w[1]; rows[b].raw_len = w[2];
    }
    if (use_ev) {
      if (w[3] < 0 || w[4] < 0) return fail(h, RV_EINVAL, "window row %d: negative event start or length (%d, %d)", b, w[3], w[4]);
      if ((long long)w[3] + w[4] > (long long)r->n_ev) return fail(h, RV_EINVAL, "window row %d: event window [%d, %lld) ends beyond the read's %zu events", b, w[3], (long long)w[3] + w[4], r->n_ev);
      if (w[4] > T_e) return fail(h, RV_EINVAL, "window row %d: event_len %d exceeds T_e=%d", b, w[4], T_e);
      rows[b].ev = r->d_ev + (size_t)w[3] * 5; rows[b].ev_len = w[4];
    }
    if (std::find(ids.begin(), ids.end(), w[0]) == ids.end()) ids.push_back(w[0]);
  }
  return RV_OK;
}

// A window call as its entry point states it: device inputs (the reads), the outputs the entry point adds
int windows_call(RvContext* h, const int32_t* win, int B, int T_r, int T_e, int W, int L, std::vector<RecWindow>& rows, std::vector<int>& ids, Call& c) {
  if (!h) return RV_EINVAL;
  TRY(resolve_windows(h, win, B, T_r, T_e, rows, ids));
  c = slab_call(nullptr, nullptr, false, B, T_r, T_e, W, L);
  c.dev_in = true;
  static const RecWindow none{nullptr, nullptr, 0, 0};
  c.windows = B > 0 ? rows.data() : &none;      // (an empty slab is still a window call)
  return RV_OK;
}

// The reads an asynchronous window call uses stay put until its ticket is collected (rv_read_drop refuses)
void hold_reads(RvContext* h, int ticket, const std::vector<int>& ids) {
  for (int id : ids) if (Read* r = find_read(h, id)) r->users += 1;
  h->ticket_reads[ticket] = ids;
}
void release_reads(RvContext* h, int ticket) {
  auto it = h->ticket_reads.find(ticket);
  if (it == h->ticket_reads.end()) return;
  for (int id : it->second) if (Read* r = find_read(h, id)) r->users -= 1;
  h->ticket_reads.erase(it);
}

int put_read(RvContext* h, const float* raw, size_t n_raw, const float* event, size_t n_event, bool on_device, int32_t* read_id) {
  if (!h || !read_id) return RV_EINVAL;
  *read_id = -1;
  const RvConfig& c = h->cfg;
  const bool use_raw = c.mode != RV_MODE_EVENT, use_ev = c.mode != RV_MODE_RAW;
  if (!use_raw) { raw = nullptr; n_raw = 0; }
  if (!use_ev) { event = nullptr; n_event = 0; }
  if ((n_raw > 0 && !raw) || (n_event > 0 && !event)) return fail(h, RV_EINVAL, "missing read pointer for this mode");
  if (n_raw > (size_t)INT32_MAX || n_event > (size_t)INT32_MAX / 5) return fail(h, RV_EINVAL, "read too long for 32-bit window offsets");
  const size_t need_ev = n_event * 5;
  // a slot: a dropped read whose buffers hold this one (the smallest such: no device allocation), else any dropped one, else a new one
  int slot = -1;
  if (!on_device)
    for (size_t i = 0; i < h->reads.size(); ++i) {
      const Read& r = h->reads[i];
      if (r.live || !r.owned || r.cap_raw < n_raw || r.cap_ev < need_ev) continue;
      if (slot < 0 || r.cap_raw + r.cap_ev < h->reads[slot].cap_raw + h->reads[slot].cap_ev) slot = (int)i;
    }
  for (size_t i = 0; i < h->reads.size() && slot < 0; ++i) if (!h->reads[i].live && (on_device || !h->reads[i].owned)) slot = (int)i;
  for (size_t i = 0; i < h->reads.size() && slot < 0; ++i) if (!h->reads[i].live) slot = (int)i;
  if (slot < 0) {
    if ((int)h->reads.size() >= RV_READ_SLOTS) return fail(h, RV_ESTATE, "%d reads are alive: drop one first", RV_READ_SLOTS);
    h->reads.emplace_back();
    slot = (int)h->reads.size() - 1;
  }
  Read& r = h->reads[slot];
  HIPCHK(h, hipSetDevice(c.device));
  if (on_device) {
    if (r.owned) { if (r.d_raw) hipFree(r.d_raw); if (r.d_ev) hipFree(r.d_ev); r.cap_raw = r.cap_ev = 0; }
    r.owned = false;
    r.d_raw = const_cast<float*>(raw); r.d_ev = const_cast<float*>(event);
  } else {
    if (!h->copy_stream) HIPCHK(h, hipStreamCreateWithFlags(&h->copy_stream, hipStreamNonBlocking));
    if (!h->ev_put) HIPCHK(h, hipEventCreateWithFlags(&h->ev_put, hipEventDisableTiming));
    if (!r.owned) { r.d_raw = r.d_ev = nullptr; r.cap_raw = r.cap_ev = 0; r.owned = true; }
    auto grow = [&](float** p, size_t* cap, size_t need) -> int {
      if (need <= *cap) return RV_OK;
      if (*p) { hipFree(*p); *p = nullptr; *cap = 0; }
      if (hipMalloc((void**)p, need * sizeof(float)) != hipSuccess) return fail(h, RV_ENOMEM, "hipMalloc(%zu bytes) failed for a read", need * sizeof(float));
      *cap = need; h->read_allocs += 1;
      return RV_OK;
    };
    TRY(grow(&r.d_raw, &r.cap_raw, n_raw));
    TRY(grow(&r.d_ev, &r.cap_ev, need_ev));
    if (r.used) HIPCHK(h, hipEventSynchronize(h->ev_put));      // (the staging of a slot taken again: its earlier upload has left it)
    if (n_raw + need_ev > r.pin_cap) {
      if (r.pin) { hipHostFree(r.pin); r.pin = nullptr; r.pin_cap = 0; }
      HIPCHK(h, hipHostMalloc((void**)&r.pin, (n_raw + need_ev) * sizeof(float), hipHostMallocDefault));
      r.pin_cap = n_raw + need_ev;
    }
    if (n_raw) { memcpy(r.pin, raw, n_raw * sizeof(float)); HIPCHK(h, hipMemcpyAsync(r.d_raw, r.pin, n_raw * sizeof(float), hipMemcpyHostToDevice, h->copy_stream)); }
    if (need_ev) { memcpy(r.pin + n_raw, event, need_ev * sizeof(float)); HIPCHK(h, hipMemcpyAsync(r.d_ev, r.pin + n_raw, need_ev * sizeof(float), hipMemcpyHostToDevice, h->copy_stream)); }
    HIPCHK(h, hipEventRecord(h->ev_put, h->copy_stream));
    r.used = true;
  }
  r.n_raw = n_raw; r.n_ev = n_event; r.live = true; r.users = 0; r.prepped = false; r.n_win = 0;
  r.ev_id = -2; r.n_xev = 0;      // (a slot taken again: the event table a caller gave its last read is not this read's)
  h->read_gen = (h->read_gen + 1) & 0xFFFFF;
  r.id = (h->read_gen << 10) | slot;
  h->read_puts += 1;
  *read_id = r.id;
  return RV_OK;
}

// ---- reads from raw signal (rv_read_put_signals; kernels: signal_prep.hip)
// A device or pinned buffer of the signal path that only grows; device allocations count as the reads' do ("read_stats")
template <class T>
int sp_grow(RvContext* h, T** p, size_t* cap, size_t need, bool pinned = false) {
  if (need <= *cap && *p) return RV_OK;
  if (*p) { if (pinned) hipHostFree(*p); else hipFree(*p); *p = nullptr; *cap = 0; }
  const size_t bytes = std::max<size_t>(need, 1) * sizeof(T);
  const hipError_t e = pinned ? hipHostMalloc((void**)p, bytes, hipHostMallocDefault) : hipMalloc((void**)p, bytes);
  if (e != hipSuccess) { *p = nullptr; return fail(h, RV_ENOMEM, "%s(%zu bytes) failed for signal preparation", pinned ? "hipHostMalloc" : "hipMalloc", bytes); }
  *cap = need;
  if (!pinned) h->read_allocs += 1;
  return RV_OK;
}

int put_signals(RvContext* h, int n_reads, const int16_t* const* signal, const size_t* n, const RvSignalPrep* prep, int32_t* read_id,
                int32_t* n_events, int32_t* n_windows) {
  if (!h) return RV_EINVAL;
  if (!prep || !read_id || n_reads < 0 || (n_reads > 0 && (!signal || !n))) return fail(h, RV_EINVAL, "rv_read_put_signals: null argument or negative n_reads");
  for (int r = 0; r < n_reads; ++r) { read_id[r] = -1; if (n_events) n_events[r] = 0; if (n_windows) n_windows[r] = 0; }
  const RvSignalPrep& q = *prep;
  if (q.window_length1 < 1 || q.window_length2 < q.window_length1 || q.window_length2 > (1 << 20))
    return fail(h, RV_EINVAL, "window lengths (%d, %d): 1 <= window_length1 <= window_length2 is needed", q.window_length1, q.window_length2);
  if (q.stride < 1) return fail(h, RV_EINVAL, "stride %d < 1", q.stride);
  if (q.max_raw_len < 1 || q.max_event_len < 1) return fail(h, RV_EINVAL, "max_raw_len %d / max_event_len %d < 1", q.max_raw_len, q.max_event_len);
  for (int r = 0; r < n_reads; ++r) {
    if (n[r] > (size_t)SP_MAX_SAMPLES)
      return fail(h, RV_EUNSUPPORTED, "read %d has %zu samples; device preparation takes up to %d (2^22): beyond that the running sums of x^2 are "
                  "no longer exact in fp64, which its bit equality with the host detector rests on -- use the host path (rv_read_put)", r, n[r], SP_MAX_SAMPLES);
    if (n[r] > 0 && !signal[r]) return fail(h, RV_EINVAL, "read %d: null signal with %zu samples", r, n[r]);
  }
  int alive = 0;
  for (const Read& r : h->reads) alive += r.live ? 1 : 0;
  if (alive + n_reads > RV_READ_SLOTS)
    return fail(h, RV_ESTATE, "%d reads are alive and %d more were put: at most %d at once, drop some first", alive, n_reads, RV_READ_SLOTS);
  if (n_reads == 0) return RV_OK;

  const RvConfig& c = h->cfg;
  HIPCHK(h, hipSetDevice(c.device));
  if (!h->copy_stream) HIPCHK(h, hipStreamCreateWithFlags(&h->copy_stream, hipStreamNonBlocking));
  if (!h->ev_put) HIPCHK(h, hipEventCreateWithFlags(&h->ev_put, hipEventDisableTiming));
  hipStream_t s = h->copy_stream;
  SignalScratch& sp = h->sp;

  // the batch's layout: a read takes n + 1 entries of the per-sample arrays (rounded up to 8) and ceil(n / SP_TILE) tiles
  std::vector<SpRead> rd((size_t)n_reads, SpRead{});
  size_t total = 0; int tiles = 0, max_tiles = 0;
  for (int r = 0; r < n_reads; ++r) {
    rd[r].off = (long long)total; rd[r].n = (int)n[r]; rd[r].tile0 = tiles; rd[r].ntile = (int)((n[r] + SP_TILE - 1) / SP_TILE);
    total += (n[r] + 1 + 7) / 8 * 8; tiles += rd[r].ntile; max_tiles = std::max(max_tiles, rd[r].ntile);
  }
  if (total > sp.cap_x) {      // (a group of buffers grows together; a failure leaves its capacity at 0, so that the next call starts over)
    const size_t old = sp.cap_x;
    size_t cap;
    sp.cap_x = 0;
    cap = old; TRY(sp_grow(h, &sp.d_x, &cap, total));
    cap = old; TRY(sp_grow(h, &sp.pin_x, &cap, total, true));
    cap = old; TRY(sp_grow(h, &sp.ps, &cap, total));
    cap = old; TRY(sp_grow(h, &sp.pq, &cap, total));
    cap = old; TRY(sp_grow(h, &sp.t1, &cap, total));
    cap = old; TRY(sp_grow(h, &sp.t2, &cap, total));
    cap = old; TRY(sp_grow(h, &sp.bounds, &cap, total));
    sp.cap_x = total;
  }
  if ((size_t)tiles > sp.cap_tiles || !sp.tile_sums) {
    const size_t old = sp.cap_tiles;
    size_t cap;
    sp.cap_tiles = 0;
    cap = old; TRY(sp_grow(h, &sp.tile_sums, &cap, 2 * (size_t)tiles));
    cap = old; TRY(sp_grow(h, &sp.var_part, &cap, (size_t)tiles));
    sp.cap_tiles = (size_t)tiles;
  }
  if ((size_t)n_reads > sp.cap_reads) {
    const size_t old = sp.cap_reads;
    size_t cap;
    sp.cap_reads = 0;
    cap = old; TRY(sp_grow(h, &sp.d_reads, &cap, (size_t)n_reads));
    cap = old; TRY(sp_grow(h, &sp.pin_reads, &cap, (size_t)n_reads, true));
    cap = old; TRY(sp_grow(h, &sp.d_cnt, &cap, 2 * (size_t)n_reads));
    cap = old; TRY(sp_grow(h, &sp.pin_cnt, &cap, 2 * (size_t)n_reads, true));
    cap = old; TRY(sp_grow(h, &sp.fit, &cap, (size_t)SP_FIT * n_reads));
    sp.cap_reads = (size_t)n_reads;
  }
  const SpScratch sc{sp.d_x, sp.ps, sp.pq, sp.t1, sp.t2, sp.bounds, sp.tile_sums, sp.var_part, sp.d_cnt, sp.d_cnt + n_reads, sp.fit};
  const SpParams pr{q.window_length1, q.window_length2, q.threshold1, q.threshold2, q.peak_height, q.stride, q.max_raw_len, q.max_event_len};

  // per-stage device times under option "profile" (scopes "sp_*")
  struct Stage { const char* name; hipEvent_t a, b; };
  std::vector<Stage> stages;
  const bool prof = h->opt.profile != 0;
  auto stage = [&](const char* name, auto&& body) {
    hipEvent_t a = nullptr, b = nullptr;
    if (prof) { hipEventCreate(&a); hipEventCreate(&b); hipEventRecord(a, s); }
    body();
    if (prof) { hipEventRecord(b, s); stages.push_back({name, a, b}); }
  };
  auto drain = [&]() {
    for (Stage& g : stages) {
      float ms = 0.f;
      if (hipEventElapsedTime(&ms, g.a, g.b) == hipSuccess) { ProfEntry& e = h->prof[g.name]; e.ms += ms; e.n += 1; }
      hipEventDestroy(g.a); hipEventDestroy(g.b);
    }
    stages.clear();
  };

  // the slots: a dropped read whose sample buffer holds this one (the smallest such), else any dropped one, else a new one.  Taken now,
  // given back if anything below fails: the call makes all its reads or none
  std::vector<int> slots;
  auto give_back = [&](int code) { for (int sl : slots) h->reads[sl].live = false; drain(); return code; };
#define SPCHK(expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) return give_back(fail(h, RV_EHIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__)); } while (0)
#define SPTRY(x) do { int r_ = (x); if (r_ != RV_OK) return give_back(r_); } while (0)
  for (int r = 0; r < n_reads; ++r) {
    int slot = -1;
    for (size_t i = 0; i < h->reads.size(); ++i) {
      const Read& x = h->reads[i];
      if (x.live || !x.owned || x.cap_raw < n[r]) continue;
      if (slot < 0 || x.cap_raw < h->reads[slot].cap_raw) slot = (int)i;
    }
    for (size_t i = 0; i < h->reads.size() && slot < 0; ++i) if (!h->reads[i].live && !h->reads[i].owned) slot = (int)i;
    for (size_t i = 0; i < h->reads.size() && slot < 0; ++i) if (!h->reads[i].live) slot = (int)i;
    if (slot < 0) { h->reads.emplace_back(); slot = (int)h->reads.size() - 1; }      // (room for it: checked above)
    Read& x = h->reads[slot];
    if (!x.owned) { x.d_raw = x.d_ev = nullptr; x.cap_raw = x.cap_ev = 0; x.owned = true; }
    x.live = true; x.users = 0; x.ev_id = -2; x.n_xev = 0;
    slots.push_back(slot);
  }

  for (int r = 0; r < n_reads; ++r) if (n[r]) memcpy(sp.pin_x + rd[r].off, signal[r], n[r] * sizeof(int16_t));
  memcpy(sp.pin_reads, rd.data(), (size_t)n_reads * sizeof(SpRead));
  hipError_t up = hipSuccess;
  stage("sp_upload", [&]() {
    up = hipMemcpyAsync(sp.d_x, sp.pin_x, total * sizeof(int16_t), hipMemcpyHostToDevice, s);
    if (up == hipSuccess) up = hipMemcpyAsync(sp.d_reads, sp.pin_reads, (size_t)n_reads * sizeof(SpRead), hipMemcpyHostToDevice, s);
    if (up == hipSuccess) up = hipMemsetAsync(sp.d_cnt, 0, 2 * (size_t)n_reads * sizeof(int), s);
  });
  SPCHK(up);
  stage("sp_scan", [&]() { sp_launch_scan(sp.d_reads, n_reads, max_tiles, sc, s); });
  stage("sp_tstat", [&]() { sp_launch_tstat(sp.d_reads, n_reads, max_tiles, sc, pr, s); });
  stage("sp_peaks", [&]() { sp_launch_peaks(sp.d_reads, n_reads, sc, pr, s); });
  SPCHK(hipGetLastError());
  SPCHK(hipMemcpyAsync(sp.pin_cnt, sp.d_cnt, (size_t)n_reads * sizeof(int), hipMemcpyDeviceToHost, s));
  SPCHK(hipStreamSynchronize(s));

  // the event counts are known: the reads' own tables
  int max_ev = 0, max_win = 0;
  for (int r = 0; r < n_reads; ++r) {
    Read& x = h->reads[slots[r]];
    const size_t E = (size_t)sp.pin_cnt[r], K = (E + (size_t)q.stride - 1) / (size_t)q.stride;
    SPTRY(sp_grow(h, &x.d_raw, &x.cap_raw, n[r]));
    SPTRY(sp_grow(h, &x.d_ev, &x.cap_ev, E * 5));
    if (E > x.cap_evd || !x.d_est) {
      const size_t old = x.cap_evd;
      size_t cap;
      x.cap_evd = 0;
      cap = old; SPTRY(sp_grow(h, &x.d_est, &cap, E));
      cap = old; SPTRY(sp_grow(h, &x.d_eln, &cap, E));
      cap = old; SPTRY(sp_grow(h, &x.d_emu, &cap, E));
      cap = old; SPTRY(sp_grow(h, &x.d_esd, &cap, E));
      x.cap_evd = E;
    }
    SPTRY(sp_grow(h, &x.d_win, &x.cap_win, K * 4));
    SpRead& g = sp.pin_reads[r];
    g.n_ev = (int)E; g.ev_start = x.d_est; g.ev_len = x.d_eln; g.ev_mean = x.d_emu; g.ev_stdv = x.d_esd;
    g.raw_sc = x.d_raw; g.ev_sc = x.d_ev; g.win = x.d_win;
    max_ev = std::max(max_ev, (int)E); max_win = std::max(max_win, (int)K);
  }
  SPCHK(hipMemcpyAsync(sp.d_reads, sp.pin_reads, (size_t)n_reads * sizeof(SpRead), hipMemcpyHostToDevice, s));
  stage("sp_events", [&]() { sp_launch_events(sp.d_reads, n_reads, max_ev, sc, pr, s); });
  stage("sp_fit", [&]() { sp_launch_fit(sp.d_reads, n_reads, sc, s); });
  stage("sp_raw_scale", [&]() { sp_launch_raw_scale(sp.d_reads, n_reads, max_tiles, sc, s); });
  stage("sp_windows", [&]() { sp_launch_windows(sp.d_reads, n_reads, max_win, sc, pr, s); });
  SPCHK(hipGetLastError());
  SPCHK(hipMemcpyAsync(sp.pin_cnt + n_reads, sp.d_cnt + n_reads, (size_t)n_reads * sizeof(int), hipMemcpyDeviceToHost, s));
  SPCHK(hipEventRecord(h->ev_put, s));
  SPCHK(hipStreamSynchronize(s));
#undef SPCHK
#undef SPTRY
  drain();

  for (int r = 0; r < n_reads; ++r) {
    Read& x = h->reads[slots[r]];
    x.n_raw = n[r]; x.n_ev = (size_t)sp.pin_cnt[r]; x.n_win = (size_t)sp.pin_cnt[n_reads + r]; x.prepped = true; x.used = true;
    h->read_gen = (h->read_gen + 1) & 0xFFFFF;
    x.id = (h->read_gen << 10) | slots[r];
    h->read_puts += 1;
    read_id[r] = x.id;
    if (n_events) n_events[r] = (int32_t)x.n_ev;
    if (n_windows) n_windows[r] = (int32_t)x.n_win;
  }
  return RV_OK;
}

int fetch_read(RvContext* h, int read_id, int what, void* dst, size_t cap) {
  if (!h) return RV_EINVAL;
  const Read* r = find_read(h, read_id);
  if (!r) return fail(h, RV_EINVAL, "unknown read_id %d", read_id);
  if (!r->owned) return fail(h, RV_ESTATE, "read %d lives in the caller's device buffers (rv_read_put_dev): nothing to fetch", read_id);
  const void* src = nullptr; size_t bytes = 0;
  switch (what) {
    case RV_FETCH_RAW_SC: src = r->d_raw; bytes = r->n_raw * sizeof(float); break;
    case RV_FETCH_EVENTS_SC: src = r->d_ev; bytes = r->n_ev * 5 * sizeof(float); break;
    case RV_FETCH_WINDOWS: src = r->d_win; bytes = r->n_win * 4 * sizeof(int32_t); break;
    case RV_FETCH_EVENT_START: src = r->d_est; bytes = r->n_ev * sizeof(int64_t); break;
    case RV_FETCH_EVENT_LENGTH: src = r->d_eln; bytes = r->n_ev * sizeof(int64_t); break;
    case RV_FETCH_EVENT_MEAN: src = r->d_emu; bytes = r->n_ev * sizeof(double); break;
    case RV_FETCH_EVENT_STDV: src = r->d_esd; bytes = r->n_ev * sizeof(double); break;
    default: return fail(h, RV_EINVAL, "rv_read_fetch: unknown table %d", what);
  }
  if (what != RV_FETCH_RAW_SC && what != RV_FETCH_EVENTS_SC && !r->prepped)
    return fail(h, RV_ESTATE, "read %d was not made by rv_read_put_signals: it has no window table and no event arrays", read_id);
  if (bytes > cap) return fail(h, RV_EINVAL, "rv_read_fetch: the table takes %zu bytes, dst holds %zu", bytes, cap);
  if (bytes == 0) return RV_OK;
  if (!dst) return fail(h, RV_EINVAL, "rv_read_fetch: null dst");
  HIPCHK(h, hipSetDevice(h->cfg.device));
  if (h->copy_stream) HIPCHK(h, hipStreamSynchronize(h->copy_stream));      // (a read put by rv_read_put: its upload is behind this)
  HIPCHK(h, hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost));
  return RV_OK;
}

// ---- stitching by signal position (rv_stitch_*, rv_read_put_events; kernels: stitch.hip)
// A device or pinned buffer of the stitch that only grows (sp_grow without the count: "read_stats" counts allocations made for reads)
template <class T>
int st_grow(RvContext* h, T** p, size_t* cap, size_t need, bool pinned = false) {
  if (need <= *cap && *p) return RV_OK;
  if (*p) { if (pinned) hipHostFree(*p); else hipFree(*p); *p = nullptr; *cap = 0; }
  const size_t bytes = std::max<size_t>(need, 1) * sizeof(T);
  const hipError_t e = pinned ? hipHostMalloc((void**)p, bytes, hipHostMallocDefault) : hipMalloc((void**)p, bytes);
  if (e != hipSuccess) { *p = nullptr; return fail(h, RV_ENOMEM, "%s(%zu bytes) failed for a stitch", pinned ? "hipHostMalloc" : "hipMalloc", bytes); }
  *cap = need;
  return RV_OK;
}

void free_stitch_buf(RvStitchBuf* sb) {
  for (void* q : {(void*)sb->bases, (void*)sb->probs, (void*)sb->lens, (void*)sb->mv[0], (void*)sb->mv[1], (void*)sb->mv[2], (void*)sb->mv[3]})
    if (q) hipFree(q);
  delete sb;
}

void free_stitch_scratch(RvContext* h) {
  StitchScratch& t = h->st;
  for (void* q : {(void*)t.chunks, (void*)t.keep, (void*)t.off, (void*)t.tiles, (void*)t.reads, (void*)t.rows, (void*)t.read_off, (void*)t.o_bases,
                  (void*)t.o_f[0], (void*)t.o_f[1], (void*)t.o_f[2], (void*)t.o_pos, (void*)t.o_i[0], (void*)t.o_i[1], (void*)t.in_bases,
                  (void*)t.in_f[0], (void*)t.in_f[1], (void*)t.in_f[2], (void*)t.in_f[3], (void*)t.in_f[4], (void*)t.in_len}) if (q) hipFree(q);
  if (t.pin_read_off) hipHostFree(t.pin_read_off);
  t = StitchScratch{};
}

RvStitchBuf* find_stitch_buf(RvContext* h, const RvStitchBuf* sb) {
  for (RvStitchBuf* k : h->stitch_bufs) if (k == sb) return k;
  return nullptr;
}

// The event table of a read on the device: its own (rv_read_put_signals) or the caller's (rv_read_put_events)
bool read_events(const Read& r, StRead* out) {
  if (r.prepped) { *out = StRead{r.d_est, r.d_eln, (int)r.n_ev}; return true; }
  if (r.ev_id == r.id) { *out = StRead{r.d_xst, r.d_xln, (int)r.n_xev}; return true; }
  return false;
}

int put_events(RvContext* h, int read_id, const int64_t* start, const int64_t* length, size_t n_event) {
  if (!h) return RV_EINVAL;
  Read* r = find_read(h, read_id);
  if (!r) return fail(h, RV_EINVAL, "unknown read_id %d", read_id);
  if (r->prepped) return fail(h, RV_ESTATE, "read %d was made by rv_read_put_signals: its event table is on the device already", read_id);
  if (n_event > 0 && (!start || !length)) return fail(h, RV_EINVAL, "rv_read_put_events: null array");
  if (n_event > (size_t)INT32_MAX) return fail(h, RV_EINVAL, "rv_read_put_events: %zu events exceed 32-bit event indices", n_event);
  if (h->cfg.mode != RV_MODE_RAW && n_event != r->n_ev)
    return fail(h, RV_EINVAL, "rv_read_put_events: %zu events for read %d, whose event table holds %zu", n_event, read_id, r->n_ev);
  HIPCHK(h, hipSetDevice(h->cfg.device));
  if (n_event > r->cap_xev || !r->d_xst) {
    const size_t old = r->cap_xev;
    size_t cap;
    r->cap_xev = 0;
    cap = old; TRY(st_grow(h, &r->d_xst, &cap, n_event));
    cap = old; TRY(st_grow(h, &r->d_xln, &cap, n_event));
    r->cap_xev = n_event;
  }
  if (n_event) {      // (synchronous copies: the arrays are the caller's again on return, and every later stream sees them)
    HIPCHK(h, hipMemcpy(r->d_xst, start, n_event * sizeof(int64_t), hipMemcpyHostToDevice));
    HIPCHK(h, hipMemcpy(r->d_xln, length, n_event * sizeof(int64_t), hipMemcpyHostToDevice));
  }
  r->n_xev = n_event; r->ev_id = r->id;
  return RV_OK;
}

// The stitch of rows read_rows[0] .. read_rows[n_reads] of the device tables `din` (n rows in all), whose window rows `win` [n,5] are on
// the host: checked there before anything is queued, then the three stages on the handle's copy stream (behind every upload of a read or
// of its events), the read offsets, and -- when they fit `out` -- the outputs
int stitch_core(RvContext* h, StIn din, const int32_t* win, int n_reads, const int32_t* read_rows, const RvStitchOut* out, const char* what) {
  if (!out || !out->read_offsets) return fail(h, RV_EINVAL, "%s: null read_offsets", what);
  if (n_reads < 0 || !read_rows) return fail(h, RV_EINVAL, "%s: null read_rows or negative n_reads", what);
  for (int r = 0; r <= n_reads; ++r)
    if (read_rows[r] < 0 || read_rows[r] > din.n || (r > 0 && read_rows[r] < read_rows[r - 1]))
      return fail(h, RV_EINVAL, "%s: read_rows[%d] = %d lies outside the table's %d rows or below the entry before it", what, r, read_rows[r], din.n);
  const int r0 = read_rows[0], n = read_rows[n_reads] - r0;
  const bool use_ev = h->cfg.mode != RV_MODE_RAW;
  std::vector<StChunk> chunks((size_t)n);
  std::vector<StRead> reads((size_t)std::max(n_reads, 1), StRead{nullptr, nullptr, 0});
  std::vector<int32_t> rows((size_t)n_reads + 1);
  for (int r = 0; r <= n_reads; ++r) rows[r] = read_rows[r] - r0;
  for (int r = 0; r < n_reads; ++r) {
    const int a = read_rows[r], b = read_rows[r + 1];
    for (int row = a; row < b; ++row) {
      const int32_t* w = win + (size_t)row * 5;
      const Read* rd = find_read(h, w[0]);
      if (!rd) return fail(h, RV_EINVAL, "%s: row %d: unknown read_id %d", what, row, w[0]);
      if (w[0] != win[(size_t)a * 5]) return fail(h, RV_EINVAL, "%s: row %d names read %d, but lies in the rows [%d,%d) of read %d", what, row, w[0], a, b, win[(size_t)a * 5]);
      if (row == a && use_ev && !read_events(*rd, &reads[r]))
        return fail(h, RV_ESTATE, "%s: read %d has no event table on the device, which the positions of this mode need: give it with rv_read_put_events", what, w[0]);
      chunks[(size_t)(row - r0)] = StChunk{w[1], w[2], w[3], w[4], r, row - a, b - a};
    }
  }

  HIPCHK(h, hipSetDevice(h->cfg.device));
  if (!h->copy_stream) HIPCHK(h, hipStreamCreateWithFlags(&h->copy_stream, hipStreamNonBlocking));
  hipStream_t s = h->copy_stream;
  StitchScratch& t = h->st;
  const int ntile = n / ST_THREADS + 1;
  TRY(st_grow(h, &t.chunks, &t.cap_chunks, (size_t)n));
  TRY(st_grow(h, &t.keep, &t.cap_keep, (size_t)n));
  TRY(st_grow(h, &t.off, &t.cap_off, (size_t)n + 1));
  TRY(st_grow(h, &t.tiles, &t.cap_tiles, (size_t)ntile));
  TRY(st_grow(h, &t.reads, &t.cap_reads, reads.size()));
  TRY(st_grow(h, &t.rows, &t.cap_rows, rows.size()));
  TRY(st_grow(h, &t.read_off, &t.cap_read_off, rows.size()));
  TRY(st_grow(h, &t.pin_read_off, &t.cap_pin, rows.size(), true));

  // per-stage device times under option "profile" (scopes "stitch_*")
  struct Stage { const char* name; hipEvent_t a, b; };
  std::vector<Stage> stages;
  const bool prof = h->opt.profile != 0;
  auto stage = [&](const char* name, auto&& body) {
    hipEvent_t a = nullptr, b = nullptr;
    if (prof) { hipEventCreate(&a); hipEventCreate(&b); hipEventRecord(a, s); }
    body();
    if (prof) { hipEventRecord(b, s); stages.push_back({name, a, b}); }
  };
  auto drain = [&](int code) {      // (behind a synchronise of the stream, or on the way out of a failure)
    for (Stage& g : stages) {
      float ms = 0.f;
      if (code == RV_OK && hipEventElapsedTime(&ms, g.a, g.b) == hipSuccess) { ProfEntry& e = h->prof[g.name]; e.ms += ms; e.n += 1; }
      hipEventDestroy(g.a); hipEventDestroy(g.b);
    }
    stages.clear();
    return code;
  };
#define STCHK(expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) return drain(fail(h, RV_EHIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__)); } while (0)

  const size_t at = (size_t)r0 * din.stride;
  din.bases += at; din.probs += at; din.raw_pos += at; din.raw_mass += at; din.event_pos += at; din.event_mass += at; din.lengths += r0;
  din.n = n; din.mode = h->cfg.mode;
  // (synchronous copies from these vectors, which go when the call returns: the stream's kernels are queued behind them)
  if (n) STCHK(hipMemcpy(t.chunks, chunks.data(), sizeof(StChunk) * (size_t)n, hipMemcpyHostToDevice));
  STCHK(hipMemcpy(t.reads, reads.data(), sizeof(StRead) * reads.size(), hipMemcpyHostToDevice));
  STCHK(hipMemcpy(t.rows, rows.data(), sizeof(int32_t) * rows.size(), hipMemcpyHostToDevice));
  stage("stitch_keep", [&]() { st_launch_keep(din, t.chunks, t.reads, t.keep, s); });
  stage("stitch_scan", [&]() { st_launch_scan(t.keep, n, t.tiles, t.off, t.rows, n_reads, t.read_off, s); });
  STCHK(hipGetLastError());
  STCHK(hipMemcpyAsync(t.pin_read_off, t.read_off, sizeof(long long) * rows.size(), hipMemcpyDeviceToHost, s));
  STCHK(hipStreamSynchronize(s));
  const long long total = t.pin_read_off[n_reads];
  for (int r = 0; r <= n_reads; ++r) out->read_offsets[r] = (int64_t)t.pin_read_off[r];
  if (total < 0 || (size_t)total > out->capacity)
    return drain(fail(h, RV_EINVAL, "%s: the reads hold %lld bases, the outputs have room for %zu", what, total, out->capacity));
  if (total > 0) {
    const size_t m = (size_t)total;
    StOut o{};
    if (out->bases) { if (int rc = st_grow(h, &t.o_bases, &t.cap_o_bases, m)) return drain(rc); o.bases = t.o_bases; }
    float** of[3] = {&o.probs, &o.raw_mass, &o.event_mass};
    float* const hf[3] = {out->probs, out->raw_mass, out->event_mass};
    for (int i = 0; i < 3; ++i) if (hf[i]) { if (int rc = st_grow(h, &t.o_f[i], &t.cap_o_f[i], m)) return drain(rc); *of[i] = t.o_f[i]; }
    if (out->positions) { if (int rc = st_grow(h, &t.o_pos, &t.cap_o_pos, m)) return drain(rc); o.positions = t.o_pos; }
    int32_t** oi[2] = {&o.source_chunk, &o.source_index};
    int32_t* const hi[2] = {out->source_chunk, out->source_index};
    for (int i = 0; i < 2; ++i) if (hi[i]) { if (int rc = st_grow(h, &t.o_i[i], &t.cap_o_i[i], m)) return drain(rc); *oi[i] = t.o_i[i]; }
    stage("stitch_scatter", [&]() { st_launch_scatter(din, t.chunks, t.reads, t.keep, t.off, o, s); });
    STCHK(hipGetLastError());
    if (o.bases) STCHK(hipMemcpyAsync(out->bases, o.bases, m, hipMemcpyDeviceToHost, s));
    for (int i = 0; i < 3; ++i) if (hf[i]) STCHK(hipMemcpyAsync(hf[i], *of[i], sizeof(float) * m, hipMemcpyDeviceToHost, s));
    if (o.positions) STCHK(hipMemcpyAsync(out->positions, o.positions, sizeof(double) * m, hipMemcpyDeviceToHost, s));
    for (int i = 0; i < 2; ++i) if (hi[i]) STCHK(hipMemcpyAsync(hi[i], *oi[i], sizeof(int32_t) * m, hipMemcpyDeviceToHost, s));
    STCHK(hipStreamSynchronize(s));
  }
#undef STCHK
  return drain(RV_OK);
}

// One host image to the device (rv_load_weights), in pieces of 1 MiB: the runtime stages a copy from pageable memory of up to a few MiB
// through its own pinned buffer, and pins the pages of a larger one first, which takes longer than the copy
int upload_image(RvContext* h, void* dst, const void* src, size_t bytes) {
  const size_t piece = (size_t)1 << 20;
  for (size_t at = 0; at < bytes; at += piece)
    HIPCHK(h, hipMemcpy((char*)dst + at, (const char*)src + at, std::min(piece, bytes - at), hipMemcpyHostToDevice));
  return RV_OK;
}

// rv_set_option on a GRU handle: the values no GRU kernel stands behind
int refuse_gru_option(RvContext* h, const char* key, int value) {
  const bool bad = (!strcmp(key, "weight_parts") && value == 1) || (!strcmp(key, "wide_recurrence") && value != 1) ||
                   (!strcmp(key, "lane_projection") && value == 0) || (!strcmp(key, "slab_graph") && value != 0);
  if (!bad) return RV_OK;
  return fail(h, RV_EUNSUPPORTED, "%s %d is not served on a bigru handle: its encoders run the sixteen-chunk matrix-pipe GRU recurrence with the "
              "layer-0 projection in the lane, its weights keep two f16 parts, and its decode runs per step outside a slab graph", key, value);
}

// Option "gru_persistent" 1 on a GRU handle: the images of k_dec_persist_gru and every context's projected-memory buffer, allocated
// on first use; the images built from `blob` (host; null: the device copy of the weights in force, copied back)
int build_gru_persist(RvContext* h, const float* blob) {
  GruPersistDev& gi = h->gimg;
  HIPCHK(h, hipSetDevice(h->cfg.device));
  if (!gi.allocated) {
#define X(T, name, count) if (!gi.name) TRY(dalloc(h, &gi.name, (count)));      /* (a retry after a failed allocation keeps what it has) */
    using wimg::E; using wimg::U; using wimg::MAX_VOCAB;
    RV_GRU_PERSIST_IMAGES(X)
#undef X
    gi.allocated = true;
  }
  for (SlabCtx* cx : h->slabs)      // (contexts created from here on allocate theirs: alloc_slab_buffers)
    if (!cx->mem2) {
      const RvConfig& c = h->cfg;
      const size_t Tm = (c.mode != RV_MODE_EVENT ? c.max_raw_len : 0) + (c.mode != RV_MODE_RAW ? c.max_event_len : 0);
      TRY(dalloc(cx, &cx->mem2, (size_t)cx->cap * Tm * RV_E));
    }
  std::vector<float> back;
  if (!blob) {
    back.resize(h->n_w);
    HIPCHK(h, hipMemcpy(back.data(), h->d_w, h->n_w * sizeof(float), hipMemcpyDeviceToHost));
    blob = back.data();
  }
  const wimg::GruPersistImages im = wimg::build_gru_persist_images(h->cfg, blob);
  gi.scales = im.scales;
#define X(T, name, count) TRY(upload_image(h, gi.name, im.name.data(), im.name.size() * sizeof(T)));
  RV_GRU_PERSIST_IMAGES(X)
#undef X
  gi.built = true;
  return RV_OK;
}

}  // namespace

// Loading the library is the earliest point a C caller reaches: ask the HIP runtime for 16 hardware queues (the asynchronous calls keep up
// to 16 slab contexts = streams in flight) unless the environment already says something, or RAVVENT_KEEP_ENV opts out.  It takes effect
// when the runtime starts (the process's first HIP call); rv_set_option("async_depth") reports when the setting in force is too small.
__attribute__((constructor)) static void rv_default_hw_queues() {
  if (!getenv("RAVVENT_KEEP_ENV")) setenv("GPU_MAX_HW_QUEUES", "16", 0);
}

extern "C" {

int rv_abi_version(void) { return RV_ABI_VERSION; }

const char* rv_last_error(rv_handle h) { return h ? h->err.c_str() : g_create_error.c_str(); }

int rv_create(const RvConfig* cfg, rv_handle* out) { return rv_create_rnn(cfg, RV_RNN_BILSTM, out); }

int rv_create_rnn(const RvConfig* cfg, int32_t rnn, rv_handle* out) {
  if (!cfg || !out) return fail(nullptr, RV_EINVAL, "null argument");
  *out = nullptr;
  const RvConfig& c = *cfg;
  if (rnn != RV_RNN_BILSTM && rnn != RV_RNN_BIGRU)
    return fail(nullptr, RV_EUNSUPPORTED, "rnn %d: RV_RNN_BILSTM (0) and RV_RNN_BIGRU (1) are built; the unidirectional families are not", (int)rnn);
  const bool gru = rnn == RV_RNN_BIGRU;
  if (c.enc_units != RV_U || c.dec_units != RV_U)
    return fail(nullptr, RV_EUNSUPPORTED, "this build is specialised for enc_units = dec_units = 128 (got %d, %d)", c.enc_units, c.dec_units);
  if (c.dec_depth < 1 || c.dec_depth > 4)
    return fail(nullptr, RV_EUNSUPPORTED, "decoder_depth %d outside [1,4]", c.dec_depth);
  if (c.enc_depth < 1 || c.enc_depth > 8) return fail(nullptr, RV_EINVAL, "encoder_depth %d outside [1,8]", c.enc_depth);
  if (c.vocab < 2 || c.vocab > RV_MAX_VOCAB) return fail(nullptr, RV_EINVAL, "vocab %d outside [2,%d]", c.vocab, RV_MAX_VOCAB);
  if (c.mode < 0 || c.mode > 2 || c.attention < 0 || c.attention > 1) return fail(nullptr, RV_EINVAL, "bad mode/attention");
  if (c.max_beam < 1 || c.max_beam > RV_MAX_BEAM) return fail(nullptr, RV_EINVAL, "max_beam %d outside [1,%d]", c.max_beam, RV_MAX_BEAM);
  if (c.max_batch < 1 || c.max_raw_len < 1 || c.max_event_len < 1 || c.max_output_len < 1)
    return fail(nullptr, RV_EINVAL, "maximum shapes must be positive");
  for (int t : {c.start_token, c.end_token, c.pad_token})
    if (t < 0 || t >= c.vocab) return fail(nullptr, RV_EINVAL, "token id %d outside vocab", t);

  if (gru) {   // k_gru_rec_mx stages the input windows of its sixteen chunks in LDS
    if (c.mode != RV_MODE_EVENT && !gru_rec_mx_window_fits(c.max_raw_len, 1))
      return fail(nullptr, RV_EUNSUPPORTED, "bigru: max_raw_len %d exceeds the 160 KB of LDS the layer-0 recurrence stages its sixteen input windows in", c.max_raw_len);
    if (c.mode != RV_MODE_RAW && !gru_rec_mx_window_fits(c.max_event_len, 5))
      return fail(nullptr, RV_EUNSUPPORTED, "bigru: max_event_len %d exceeds the 160 KB of LDS the layer-0 recurrence stages its sixteen input windows in", c.max_event_len);
  } else {   // layer 0 keeps a workgroup's input windows in LDS (160 KB): reject maximum shapes no kernel variant can launch
    const int bt = pick_rows_per_block(c.max_batch);
    if (c.mode != RV_MODE_EVENT && !lstm_rec_window_fits(1, bt, c.max_raw_len))
      return fail(nullptr, RV_EUNSUPPORTED, "max_raw_len %d with max_batch %d (%d chunks per workgroup) exceeds the 160 KB of LDS the layer-0 recurrence stages its input windows in", c.max_raw_len, c.max_batch, bt);
    if (c.mode != RV_MODE_RAW && !lstm_rec_window_fits(5, bt, c.max_event_len))
      return fail(nullptr, RV_EUNSUPPORTED, "max_event_len %d with max_batch %d (%d chunks per workgroup) exceeds the 160 KB of LDS the layer-0 recurrence stages its input windows in", c.max_event_len, c.max_batch, bt);
  }
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
    return fail(nullptr, RV_EHIP, "no HIP device visible: libravvent_hip has no CPU path");
  if (c.device < 0 || c.device >= ndev) return fail(nullptr, RV_EINVAL, "device %d outside [0,%d)", c.device, ndev);

  RvContext* h = new RvContext();
  h->cfg = c;
  h->rnn = rnn;
  auto init = [&]() -> int {
  HIPTRY(hipSetDevice(c.device));
  HIPTRY(configure_decode_kernels());    // a refused LDS opt-in would otherwise surface as an opaque launch error later
  if (!gru) {                            // (a GRU handle launches neither LSTM recurrence)
    HIPTRY(configure_rec_kernels());
    HIPTRY(configure_mx_kernels());
  }
  HIPTRY(configure_gemm_kernels());
  h->n_w = wimg::BlobLayout(c, rnn).total;
  TRY(dalloc(h, &h->d_w, h->n_w));
  if (gru) HIPTRY(configure_gru_kernels());
  const wimg::ImageCounts cnt = wimg::image_counts(c, rnn);
#define X(T, name, count) if (cnt.name) TRY(dalloc(h, &h->img.name, cnt.name));
  RV_WEIGHT_IMAGES(X)
#undef X
#ifdef RV_DIAG
  if (const char* e = getenv("RV_DBG_ROLE")) h->dbg_role = atoi(e);
#endif
  if (const char* e = getenv("RV_DECODE_SPLIT")) h->opt.split = atoi(e);
  bind_weights(h);
  SlabCtx* own = nullptr;
  TRY(create_slab(h, &own, c.max_batch, 0));
  h->slabs.push_back(own);
  return RV_OK;
  };
  const int rc = init();
  if (rc != RV_OK) { g_create_error = h->err; rv_destroy(h); return rc; }
  *out = h;
  return RV_OK;
}

void rv_destroy(rv_handle h) {
  if (!h) return;
  hipSetDevice(h->cfg.device);
  for (size_t i = 1; i < h->slabs.size(); ++i) destroy_slab(h->slabs[i]);
  for (Group* g : h->groups) destroy_group(g);
  if (!h->slabs.empty()) destroy_slab(h->slabs[0]);
  for (void* p : h->allocs) hipFree(p);      // (behind every stream that read the weights)
  for (Read& r : h->reads) {
    if (r.owned) { if (r.d_raw) hipFree(r.d_raw); if (r.d_ev) hipFree(r.d_ev); }
    if (r.pin) hipHostFree(r.pin);
    for (void* q : {(void*)r.d_est, (void*)r.d_eln, (void*)r.d_emu, (void*)r.d_esd, (void*)r.d_win, (void*)r.d_xst, (void*)r.d_xln}) if (q) hipFree(q);
  }
  for (RvStitchBuf* sb : h->stitch_bufs) free_stitch_buf(sb);
  free_stitch_scratch(h);
  {
    SignalScratch& sp = h->sp;
    for (void* q : {(void*)sp.d_x, (void*)sp.ps, (void*)sp.pq, (void*)sp.t1, (void*)sp.t2, (void*)sp.bounds, (void*)sp.tile_sums, (void*)sp.var_part,
                    (void*)sp.d_reads, (void*)sp.d_cnt, (void*)sp.fit}) if (q) hipFree(q);
    for (void* q : {(void*)sp.pin_x, (void*)sp.pin_reads, (void*)sp.pin_cnt}) if (q) hipHostFree(q);
  }
  if (h->copy_stream) { hipStreamSynchronize(h->copy_stream); hipStreamDestroy(h->copy_stream); }
  if (h->ev_put) hipEventDestroy(h->ev_put);
  delete h;
}

size_t rv_weight_count(rv_handle h) { return h ? h->n_w : 0; }

int rv_round_weights(const RvConfig* cfg, const float* src, float* dst, size_t n_floats) {
  if (!cfg || !src || !dst) return RV_EINVAL;
  const RvConfig& c = *cfg;
  if (c.enc_units != RV_U || c.dec_units != RV_U || c.dec_depth < 1 || c.dec_depth > 4 || c.enc_depth < 1 || c.enc_depth > 8 ||
      c.vocab < 2 || c.vocab > RV_MAX_VOCAB || n_floats != wimg::BlobLayout(c, RV_RNN_BILSTM).total) return RV_EINVAL;
  if (dst != src) memmove(dst, src, n_floats * sizeof(float));
  wimg::round_blob_weights(c, dst);
  return RV_OK;
}

int rv_load_weights(rv_handle h, const float* blob, size_t n_floats) {
  if (!h) return RV_EINVAL;
  if (!blob) return fail(h, RV_EINVAL, "null weight blob");
  if (n_floats != h->n_w) return fail(h, RV_EINVAL, "weight blob has %zu floats, config needs %zu", n_floats, h->n_w);
  flush_open_group(h);
  if (uncollected(h)) return fail(h, RV_ESTATE, "collect the calls in flight before loading weights");
  HIPCHK(h, hipSetDevice(h->cfg.device));
  h->opt.gen++;                      // (weight-derived scalars travel by value in the decode's kernel arguments)
  // weight_parts 1: every image -- and the device copy of the blob -- is built from the blob with its blob-level tensors rounded
  std::vector<float> rounded;
  if (h->opt.weight_parts == 1) {
    rounded.assign(blob, blob + n_floats);
    wimg::round_blob_weights(h->cfg, rounded.data());
    blob = rounded.data();
  }
  h->opt.parts_loaded = h->opt.weight_parts;
  hipStream_t s = h->slabs[0]->stream;
  HIPCHK(h, hipMemcpyAsync(h->d_w, blob, n_floats * sizeof(float), hipMemcpyHostToDevice, s));
  const wimg::HostImages im = wimg::build_weight_images(h->cfg, h->rnn, h->opt.weight_parts, blob);
  h->scales = im.scales;
#define X(T, name, count) TRY(upload_image(h, h->img.name, im.name.data(), im.name.size() * sizeof(T)));
  RV_WEIGHT_IMAGES(X)
#undef X
  HIPCHK(h, hipStreamSynchronize(s));
  h->gimg.built = false;
  if (h->opt.gru_persist) TRY(build_gru_persist(h, blob));
  h->loaded = true;
  return RV_OK;
}

int rv_beam_search(rv_handle h, const float* raw, const float* event, int32_t B, int32_t T_r, int32_t T_e,
                   int32_t W, int32_t L, int32_t* tokens, float* scores, int32_t* S_out) {
  Call c = slab_call(raw, event, false, B, T_r, T_e, W, L);
  c.tokens = tokens; c.out2 = scores;
  return run(h, c, S_out);
}
int rv_beam_search_dev(rv_handle h, const float* raw, const float* event, int32_t B, int32_t T_r, int32_t T_e,
                       int32_t W, int32_t L, int32_t* tokens, float* scores, int32_t* S_out) {
  Call c = slab_call(raw, event, true, B, T_r, T_e, W, L);
  c.tokens = tokens; c.out2 = scores;
  return run(h, c, S_out);
}
int rv_beam_search_calls(rv_handle h, const float* raw, const float* event, int32_t B, int32_t T_r, int32_t T_e,
                         int32_t W, int32_t L, const uint8_t* lut, uint8_t* bases, int32_t* lengths, float* probs,
                         int32_t* S_out) {
  const CallsOut co{lut, bases, lengths, probs};
  Call c = slab_call(raw, event, false, B, T_r, T_e, W, L);
  c.lut = lut; c.calls = &co;
  return run(h, c, S_out);
}
int rv_greedy_search(rv_handle h, const float* raw, const float* event, int32_t B, int32_t T_r, int32_t T_e,
                     int32_t L, int32_t* tokens, float* logits, int32_t* S_out) {
  Call c = slab_call(raw, event, false, B, T_r, T_e, 1, L);
  c.greedy = true; c.tokens = tokens; c.out2 = logits;
  return run(h, c, S_out);
}
int rv_greedy_search_dev(rv_handle h, const float* raw, const float* event, int32_t B, int32_t T_r, int32_t T_e,
                         int32_t L, int32_t* tokens, float* logits, int32_t* S_out) {
  Call c = slab_call(raw, event, true, B, T_r, T_e, 1, L);
  c.greedy = true; c.tokens = tokens; c.out2 = logits;
  return run(h, c, S_out);
}

// Decoder.call under TrainingSampler, as _train_step drives it: greedy decode's launches with the labels fed in, then k_score_tokens
int rv_teacher_forced(rv_handle h, const float* raw, const float* event, int32_t B, int32_t T_r, int32_t T_e, int32_t L,
                      const int32_t* targets, uint32_t omit_mask, int32_t* sample_id, float* logits, const RvScore* out) {
  const ForcedCall fc{targets, omit_mask, out};
  Call c = slab_call(raw, event, false, B, T_r, T_e, 1, L);
  c.greedy = true; c.tokens = sample_id; c.out2 = logits; c.forced = &fc;
  int32_t S = 0;
  return run(h, c, &S);
}
int rv_teacher_forced_dev(rv_handle h, const float* raw, const float* event, int32_t B, int32_t T_r, int32_t T_e, int32_t L,
                          const int32_t* targets, uint32_t omit_mask, int32_t* sample_id, float* logits, const RvScore* out) {
  const ForcedCall fc{targets, omit_mask, out};
  Call c = slab_call(raw, event, true, B, T_r, T_e, 1, L);
  c.greedy = true; c.tokens = sample_id; c.out2 = logits; c.forced = &fc;
  int32_t S = 0;
  return run(h, c, &S);
}

// loss_function / masked_accuracy on logits the caller holds (test_step: the zero-padded greedy logits); host buffers
int rv_score_logits(rv_handle h, const float* logits, const int32_t* labels, int32_t B, int32_t S, uint32_t omit_mask, int32_t* pred,
                    const RvScore* out) {
  if (!h) return RV_EINVAL;
  const RvConfig& c = h->cfg;
  if (B < 0 || B > c.max_batch) return fail(h, RV_EINVAL, "B=%d outside [0,%d]", B, c.max_batch);
  if (S < 0 || S > c.max_output_len || S > 64) return fail(h, RV_EINVAL, "S=%d outside [0,%d]", S, std::min(c.max_output_len, 64));
  if (B > 0 && S > 0 && (!logits || !labels)) return fail(h, RV_EINVAL, "null input pointer");
  const size_t n = (size_t)B * S;
  TRY(check_token_ids(h, labels, n, std::max(S, 1), "label"));
  SlabCtx* ctx = nullptr;
  TRY(sync_context(h, &ctx));
  if (n == 0) return fetch_scores(h, ScoreArgs{}, out, false, B, 0);
  HIPCHK(h, hipSetDevice(c.device));
  TRY(ensure_score_buffers(ctx));
  const ForcedCall fc{labels, omit_mask, out};
  HIPCHK(h, hipMemcpy(ctx->out2, logits, sizeof(float) * n * c.vocab, hipMemcpyHostToDevice));
  HIPCHK(h, hipMemcpy(ctx->d_forced, labels, sizeof(int32_t) * n, hipMemcpyHostToDevice));
  ScoreArgs a = score_outputs(ctx, &fc, false);
  a.logits = ctx->out2; a.labels = ctx->d_forced; a.label_stride = S; a.B = B; a.S = S; a.V = c.vocab; a.pad_token = c.pad_token;
  a.pred = pred ? ctx->out_tokens : nullptr;
  launch_score_tokens(a, ctx->stream);
  HIPCHK(h, hipStreamSynchronize(ctx->stream));
  HIPCHK(h, hipGetLastError());
  if (pred) HIPCHK(h, hipMemcpy(pred, ctx->out_tokens, sizeof(int32_t) * n, hipMemcpyDeviceToHost));
  return fetch_scores(h, a, out, false, B, S);
}

// ---- asynchronous calls: submit returns once the slab's work is queued on one of the handle's contexts; collect waits for it.
static int submit(rv_handle h, const Call& call, int32_t* ticket) {
  if (!h || !ticket) return RV_EINVAL;
  *ticket = -1;
  const int depth = async_depth(h);
  const int n_co = coalesce_n(h, depth);
  bool ticks_out = false;
  for (const auto& t : h->ticks) ticks_out = ticks_out || t.busy;
  if (n_co >= 2 || ticks_out) {            // (neither: the path below, one context per slab, as it always was)
    Call ok;
    TRY(validate_call(h->slabs[0], call, ok));      // (against the handle's max_batch and options as set)
    if (uncollected(h) >= depth)
      return fail(h, RV_ESTATE, "all %d asynchronous slots hold uncollected calls (option async_depth): collect one first", depth);
    h->inflight_hint = depth;
    if (n_co >= 2 && !call.whole_beam && !call.want_call_moves && coalescible(h, ok))
      return submit_group(h, n_co, ok, ticket);
    flush_open_group(h);      // a slab of another path: the group goes as it is, this slab on a context of its own
  }
  while ((int)h->slabs.size() < depth) {
    SlabCtx* k = nullptr;
    TRY(create_slab(h, &k, h->cfg.max_batch, (int)h->slabs.size()));
    h->slabs.push_back(k);
  }
  SlabCtx* ctx = nullptr; int slot = -1;
  for (int i = 0; i < depth && !ctx; ++i) {          // round robin over the idle contexts
    const int sidx = (h->next_slot + i) % depth;
    if (!h->slabs[sidx]->pend.busy) { ctx = h->slabs[sidx]; slot = sidx; }
  }
  if (!ctx) return fail(h, RV_ESTATE, "all %d asynchronous contexts hold uncollected calls (option async_depth): collect one first", depth);
  h->inflight_hint = depth;
  CallParts res;
  if (call.whole_beam) TRY(begin_all_beams(ctx, call, res));
  if (call.want_moves) TRY(begin_moves(ctx, call, res));
  if (call.want_call_moves) TRY(begin_call_moves(ctx, call, res));
  const int rc = enqueue(ctx, call, res);
  if (rc != RV_OK) { ctx->pend.busy = false; return rc; }
  h->next_slot = (slot + 1) % depth;
  ctx->pend.ticket = issue_ticket(h, slot);
  *ticket = ctx->pend.ticket;
  return RV_OK;
}
static void release_stitch(RvContext* h, int ticket) {
  auto it = h->stitch_tickets.find(ticket);
  if (it == h->stitch_tickets.end()) return;
  it->second->tickets -= 1;
  h->stitch_tickets.erase(it);
}
static int collect(rv_handle h, int32_t ticket, int32_t* tokens, float* out2, const CallsOut* calls, int32_t* S_out, const RvBeams* beams = nullptr,
                   const RvMoves* moves = nullptr, const RvCallMoves* cmoves = nullptr, bool stitch = false) {
  if (!h || !S_out) return RV_EINVAL;
  const int slot = ticket & 15;
  if (ticket >= 0 && h->ticks[slot].busy && h->ticks[slot].ticket == ticket) {
    if (moves) return fail(h, RV_EINVAL, "rv_beam_search_collect_moves takes the tickets of rv_beam_search_submit_moves");
    if (cmoves) return fail(h, RV_EINVAL, "rv_beam_search_collect_calls_moves takes the tickets of rv_beam_search_submit_windows_calls_moves");
    if (beams) return fail(h, RV_EINVAL, "rv_beam_search_collect_all takes the tickets of rv_beam_search_submit_all");      // (a group never holds one)
    if (stitch) return fail(h, RV_EINVAL, "rv_beam_search_collect_stitch takes the tickets of rv_beam_search_submit_windows_stitch");
    const int rc = collect_group(h, slot, tokens, out2, calls, S_out);
    if (!(h->ticks[slot].busy && h->ticks[slot].ticket == ticket)) release_reads(h, ticket);      // (the ticket is gone: its reads may be dropped)
    return rc;
  }
  if (ticket < 0 || slot >= (int)h->slabs.size()) return fail(h, RV_EINVAL, "unknown ticket %d", ticket);
  SlabCtx* ctx = h->slabs[slot];
  if (!ctx->pend.busy || ctx->pend.ticket != ticket) return fail(h, RV_ESTATE, "ticket %d is not in flight (collected already?)", ticket);
  const int rc = finish(ctx, tokens, out2, calls, S_out, beams, moves, cmoves, stitch);
  if (!(ctx->pend.busy && ctx->pend.ticket == ticket)) { release_reads(h, ticket); release_stitch(h, ticket); }
  return rc;
}
int rv_beam_search_submit(rv_handle h, const float* raw, const float* event, int32_t B, int32_t T_r, int32_t T_e, int32_t W, int32_t L,
                          int32_t* ticket) {
  return submit(h, slab_call(raw, event, false, B, T_r, T_e, W, L), ticket);
}
int rv_beam_search_collect(rv_handle h, int32_t ticket, int32_t* tokens, float* scores, int32_t* S_out) {
  return collect(h, ticket, tokens, scores, nullptr, S_out);
}
int rv_beam_search_submit_dev(rv_handle h, const float* d_raw, const float* d_event, int32_t B, int32_t T_r, int32_t T_e, int32_t W,
                              int32_t L, int32_t* d_tokens, float* d_scores, int32_t* ticket) {
  Call c = slab_call(d_raw, d_event, true, B, T_r, T_e, W, L);
  c.tokens = d_tokens; c.out2 = d_scores;
  return submit(h, c, ticket);
}
int rv_beam_search_collect_dev(rv_handle h, int32_t ticket, int32_t* S_out) {
  return collect(h, ticket, nullptr, nullptr, nullptr, S_out);
}
int rv_beam_search_submit_calls(rv_handle h, const float* raw, const float* event, int32_t B, int32_t T_r, int32_t T_e, int32_t W,
                                int32_t L, const uint8_t* lut, int32_t* ticket) {
  if (!lut) return h ? fail(h, RV_EINVAL, "null lut") : RV_EINVAL;
  Call c = slab_call(raw, event, false, B, T_r, T_e, W, L);
  c.lut = lut;
  return submit(h, c, ticket);
}
int rv_beam_search_collect_calls(rv_handle h, int32_t ticket, uint8_t* bases, int32_t* lengths, float* probs, int32_t* S_out) {
  const CallsOut c{nullptr, bases, lengths, probs};
  return collect(h, ticket, nullptr, nullptr, &c, S_out);
}

// ---- reads on the device, and beam search over windows of them
int rv_read_put(rv_handle h, const float* raw, size_t n_raw, const float* event, size_t n_event, int32_t* read_id) {
  return put_read(h, raw, n_raw, event, n_event, false, read_id);
}
int rv_read_put_dev(rv_handle h, const float* d_raw, size_t n_raw, const float* d_event, size_t n_event, int32_t* read_id) {
  return put_read(h, d_raw, n_raw, d_event, n_event, true, read_id);
}
int rv_read_put_signals(rv_handle h, int32_t n_reads, const int16_t* const* signal, const size_t* n, const RvSignalPrep* prep,
                        int32_t* read_id, int32_t* n_events, int32_t* n_windows) {
  return put_signals(h, n_reads, signal, n, prep, read_id, n_events, n_windows);
}
int rv_read_fetch(rv_handle h, int32_t read_id, int32_t what, void* dst, size_t cap) { return fetch_read(h, read_id, what, dst, cap); }
int rv_read_drop(rv_handle h, int32_t read_id) {
  if (!h) return RV_EINVAL;
  Read* r = find_read(h, read_id);
  if (!r) return fail(h, RV_EINVAL, "unknown read_id %d", read_id);
  if (r->users > 0) return fail(h, RV_ESTATE, "read %d is used by %d uncollected ticket(s): collect them first", read_id, r->users);
  r->live = false;
  if (!r->owned) { r->d_raw = r->d_ev = nullptr; }
  return RV_OK;
}
int rv_beam_search_windows(rv_handle h, const int32_t* win, int32_t B, int32_t T_r, int32_t T_e, int32_t W, int32_t L, int32_t* tokens,
                           float* scores, int32_t* S_out) {
  std::vector<RecWindow> rows; std::vector<int> ids; Call c;
  TRY(windows_call(h, win, B, T_r, T_e, W, L, rows, ids, c));
  c.tokens = tokens; c.out2 = scores;
  return run(h, c, S_out);
}
int rv_beam_search_windows_dev(rv_handle h, const int32_t* win, int32_t B, int32_t T_r, int32_t T_e, int32_t W, int32_t L,
                               int32_t* d_tokens, float* d_scores, int32_t* S_out) {
  std::vector<RecWindow> rows; std::vector<int> ids; Call c;
  TRY(windows_call(h, win, B, T_r, T_e, W, L, rows, ids, c));
  c.dev_out = true; c.tokens = d_tokens; c.out2 = d_scores;
  return run(h, c, S_out);
}
int rv_beam_search_windows_calls(rv_handle h, const int32_t* win, int32_t B, int32_t T_r, int32_t T_e, int32_t W, int32_t L,
                                 const uint8_t* lut, uint8_t* bases, int32_t* lengths, float* probs, int32_t* S_out) {
  std::vector<RecWindow> rows; std::vector<int> ids; Call c;
  TRY(windows_call(h, win, B, T_r, T_e, W, L, rows, ids, c));
  const CallsOut co{lut, bases, lengths, probs};
  c.lut = lut; c.calls = &co;
  return run(h, c, S_out);
}
int rv_beam_search_submit_windows(rv_handle h, const int32_t* win, int32_t B, int32_t T_r, int32_t T_e, int32_t W, int32_t L,
                                  int32_t* ticket) {
  std::vector<RecWindow> rows; std::vector<int> ids; Call c;
  TRY(windows_call(h, win, B, T_r, T_e, W, L, rows, ids, c));
  TRY(submit(h, c, ticket));
  hold_reads(h, *ticket, ids);
  return RV_OK;
}
int rv_beam_search_submit_windows_calls(rv_handle h, const int32_t* win, int32_t B, int32_t T_r, int32_t T_e, int32_t W, int32_t L,
                                        const uint8_t* lut, int32_t* ticket) {
  if (!lut) return h ? fail(h, RV_EINVAL, "null lut") : RV_EINVAL;
  std::vector<RecWindow> rows; std::vector<int> ids; Call c;
  TRY(windows_call(h, win, B, T_r, T_e, W, L, rows, ids, c));
  c.lut = lut;
  TRY(submit(h, c, ticket));
  hold_reads(h, *ticket, ids);
  return RV_OK;
}

// ---- the whole beam (k_dec_finalize_beams): tokens and scores are required, the other three outputs may be null
static bool beams_missing(const RvBeams* o, int B, int L) { return !o || (B > 0 && L > 1 && (!o->tokens || !o->scores)); }
int rv_beam_search_all(rv_handle h, const float* raw, const float* event, int32_t B, int32_t T_r, int32_t T_e, int32_t W, int32_t L,
                       const RvBeams* out, int32_t* S_out) {
  if (!h) return RV_EINVAL;
  if (beams_missing(out, B, L)) return fail(h, RV_EINVAL, "null output pointer");
  Call c = slab_call(raw, event, false, B, T_r, T_e, W, L);
  c.tokens = out->tokens; c.out2 = out->scores; c.whole_beam = true; c.beams = out;
  return run(h, c, S_out);
}
int rv_beam_search_all_dev(rv_handle h, const float* d_raw, const float* d_event, int32_t B, int32_t T_r, int32_t T_e, int32_t W,
                           int32_t L, const RvBeams* d_out, int32_t* S_out) {
  if (!h) return RV_EINVAL;
  if (beams_missing(d_out, B, L)) return fail(h, RV_EINVAL, "null output pointer");
  Call c = slab_call(d_raw, d_event, true, B, T_r, T_e, W, L);
  c.tokens = d_out->tokens; c.out2 = d_out->scores; c.whole_beam = true; c.beams = d_out;
  return run(h, c, S_out);
}
int rv_beam_search_submit_all(rv_handle h, const float* raw, const float* event, int32_t B, int32_t T_r, int32_t T_e, int32_t W,
                              int32_t L, int32_t* ticket) {
  Call c = slab_call(raw, event, false, B, T_r, T_e, W, L);
  c.whole_beam = true;
  return submit(h, c, ticket);
}
int rv_beam_search_collect_all(rv_handle h, int32_t ticket, const RvBeams* out, int32_t* S_out) {
  if (!h) return RV_EINVAL;
  if (!out) return fail(h, RV_EINVAL, "null output pointer");
  return collect(h, ticket, nullptr, nullptr, nullptr, S_out, out);
}
int rv_beam_search_submit_all_dev(rv_handle h, const float* d_raw, const float* d_event, int32_t B, int32_t T_r, int32_t T_e,
                                  int32_t W, int32_t L, const RvBeams* d_out, int32_t* ticket) {
  if (!h) return RV_EINVAL;
  if (beams_missing(d_out, B, L)) return fail(h, RV_EINVAL, "null output pointer");
  Call c = slab_call(d_raw, d_event, true, B, T_r, T_e, W, L);
  c.tokens = d_out->tokens; c.out2 = d_out->scores; c.whole_beam = true; c.beams = d_out;
  return submit(h, c, ticket);
}

// ---- the moves (k_dec_finalize_moves behind k_dec_finalize_beams): `out` as rv_beam_search_all's; every member of `moves` may be null, not all
static bool moves_missing(const RvMoves* m, int B, int L) {      // (an empty tensor has no address)
  return !m || (B > 0 && L > 1 && !m->raw_pos && !m->raw_mass && !m->event_pos && !m->event_mass && !m->peak && !m->peak_weight);
}
int rv_beam_search_moves(rv_handle h, const float* raw, const float* event, int32_t B, int32_t T_r, int32_t T_e, int32_t W, int32_t L,
                         const RvBeams* out, const RvMoves* moves, int32_t* S_out) {
  if (!h) return RV_EINVAL;
  if (beams_missing(out, B, L) || moves_missing(moves, B, L)) return fail(h, RV_EINVAL, "null output pointer");
  Call c = slab_call(raw, event, false, B, T_r, T_e, W, L);
  c.tokens = out->tokens; c.out2 = out->scores; c.whole_beam = true; c.beams = out; c.want_moves = true; c.moves = moves;
  return run(h, c, S_out);
}
int rv_beam_search_moves_dev(rv_handle h, const float* d_raw, const float* d_event, int32_t B, int32_t T_r, int32_t T_e, int32_t W,
                             int32_t L, const RvBeams* d_out, const RvMoves* d_moves, int32_t* S_out) {
  if (!h) return RV_EINVAL;
  if (beams_missing(d_out, B, L) || moves_missing(d_moves, B, L)) return fail(h, RV_EINVAL, "null output pointer");
  Call c = slab_call(d_raw, d_event, true, B, T_r, T_e, W, L);
  c.tokens = d_out->tokens; c.out2 = d_out->scores; c.whole_beam = true; c.beams = d_out; c.want_moves = true; c.moves = d_moves;
  return run(h, c, S_out);
}
int rv_beam_search_submit_moves(rv_handle h, const float* raw, const float* event, int32_t B, int32_t T_r, int32_t T_e, int32_t W,
                                int32_t L, int32_t* ticket) {
  Call c = slab_call(raw, event, false, B, T_r, T_e, W, L);
  c.whole_beam = true; c.want_moves = true;
  return submit(h, c, ticket);
}
int rv_beam_search_collect_moves(rv_handle h, int32_t ticket, const RvBeams* out, const RvMoves* moves, int32_t* S_out) {
  if (!h) return RV_EINVAL;
  if (!out || !moves) return fail(h, RV_EINVAL, "null output pointer");      // (all six null: refused at the ticket, which knows whether anything ran)
  return collect(h, ticket, nullptr, nullptr, nullptr, S_out, out, moves);
}

// ---- calls with positions (k_dec_finalize_calls_moves behind k_dec_finalize): the calls' outputs and lut as rv_beam_search_calls';
// every member of `moves` may be null, not all
static bool call_moves_missing(const RvCallMoves* m, int B, int L) {      // (an empty tensor has no address)
  return !m || (B > 0 && L > 1 && !m->raw_pos && !m->raw_mass && !m->event_pos && !m->event_mass && !m->peak && !m->peak_weight);
}
int rv_beam_search_calls_moves(rv_handle h, const float* raw, const float* event, int32_t B, int32_t T_r, int32_t T_e, int32_t W, int32_t L,
                               const uint8_t* lut, uint8_t* bases, int32_t* lengths, float* probs, const RvCallMoves* moves, int32_t* S_out) {
  if (!h) return RV_EINVAL;
  if (call_moves_missing(moves, B, L)) return fail(h, RV_EINVAL, "null output pointer");
  const CallsOut co{lut, bases, lengths, probs};
  Call c = slab_call(raw, event, false, B, T_r, T_e, W, L);
  c.lut = lut; c.calls = &co; c.want_call_moves = true; c.call_moves = moves;
  return run(h, c, S_out);
}
int rv_beam_search_windows_calls_moves(rv_handle h, const int32_t* win, int32_t B, int32_t T_r, int32_t T_e, int32_t W, int32_t L,
                                       const uint8_t* lut, uint8_t* bases, int32_t* lengths, float* probs, const RvCallMoves* moves,
                                       int32_t* S_out) {
  if (!h) return RV_EINVAL;
  if (call_moves_missing(moves, B, L)) return fail(h, RV_EINVAL, "null output pointer");
  std::vector<RecWindow> rows; std::vector<int> ids; Call c;
  TRY(windows_call(h, win, B, T_r, T_e, W, L, rows, ids, c));
  const CallsOut co{lut, bases, lengths, probs};
  c.lut = lut; c.calls = &co; c.want_call_moves = true; c.call_moves = moves;
  return run(h, c, S_out);
}
int rv_beam_search_submit_windows_calls_moves(rv_handle h, const int32_t* win, int32_t B, int32_t T_r, int32_t T_e, int32_t W, int32_t L,
                                              const uint8_t* lut, int32_t* ticket) {
  if (!lut) return h ? fail(h, RV_EINVAL, "null lut") : RV_EINVAL;
  std::vector<RecWindow> rows; std::vector<int> ids; Call c;
  TRY(windows_call(h, win, B, T_r, T_e, W, L, rows, ids, c));
  c.lut = lut; c.want_call_moves = true;
  TRY(submit(h, c, ticket));
  hold_reads(h, *ticket, ids);
  return RV_OK;
}
int rv_beam_search_collect_calls_moves(rv_handle h, int32_t ticket, uint8_t* bases, int32_t* lengths, float* probs, const RvCallMoves* moves,
                                       int32_t* S_out) {
  if (!h) return RV_EINVAL;
  if (!moves) return fail(h, RV_EINVAL, "null output pointer");      // (all six null: refused at the ticket, which knows whether anything ran)
  const CallsOut c{nullptr, bases, lengths, probs};
  return collect(h, ticket, nullptr, nullptr, &c, S_out, nullptr, nullptr, moves);
}

// ---- stitching by signal position (stitch.hip)
int rv_read_put_events(rv_handle h, int32_t read_id, const int64_t* start, const int64_t* length, size_t n_event) {
  return put_events(h, read_id, start, length, n_event);
}
int rv_stitch_calls(rv_handle h, const RvStitchIn* in, int32_t n_reads, const int32_t* read_rows, const RvStitchOut* out) {
  if (!h) return RV_EINVAL;
  if (!in || in->n < 0) return fail(h, RV_EINVAL, "rv_stitch_calls: null input or negative n");
  if (in->stride < 0 || in->stride > ST_LANES) return fail(h, RV_EINVAL, "rv_stitch_calls: row stride %d outside [0,%d]", in->stride, ST_LANES);
  const size_t n = (size_t)in->n, cells = n * (size_t)in->stride;
  if (n > 0 && (!in->lengths || !in->win)) return fail(h, RV_EINVAL, "rv_stitch_calls: null lengths or window table");
  if (cells > 0 && (!in->bases || !in->probs || !in->raw_pos || !in->raw_mass || !in->event_pos || !in->event_mass))
    return fail(h, RV_EINVAL, "rv_stitch_calls: null input array");
  HIPCHK(h, hipSetDevice(h->cfg.device));
  // the tables go up into the handle's stitch scratch (synchronous copies: the caller's arrays are free on return)
  StitchScratch& t = h->st;
  TRY(st_grow(h, &t.in_bases, &t.cap_in_bases, cells));
  TRY(st_grow(h, &t.in_len, &t.cap_in_len, n));
  const float* const src[5] = {in->probs, in->raw_pos, in->raw_mass, in->event_pos, in->event_mass};
  for (int i = 0; i < 5; ++i) TRY(st_grow(h, &t.in_f[i], &t.cap_in_f[i], cells));
  if (cells) {
    HIPCHK(h, hipMemcpy(t.in_bases, in->bases, cells, hipMemcpyHostToDevice));
    for (int i = 0; i < 5; ++i) HIPCHK(h, hipMemcpy(t.in_f[i], src[i], cells * sizeof(float), hipMemcpyHostToDevice));
  }
  if (n) HIPCHK(h, hipMemcpy(t.in_len, in->lengths, n * sizeof(int32_t), hipMemcpyHostToDevice));
  StIn d{t.in_bases, t.in_f[0], t.in_len, t.in_f[1], t.in_f[2], t.in_f[3], t.in_f[4], 0, 0, 0};
  d.n = in->n; d.stride = in->stride;
  return stitch_core(h, d, in->win, n_reads, read_rows, out, "rv_stitch_calls");
}
int rv_stitch_open(rv_handle h, int32_t n_chunks, int32_t L, rv_stitch* sb_out) {
  if (!h || !sb_out) return RV_EINVAL;
  *sb_out = nullptr;
  if (n_chunks < 0) return fail(h, RV_EINVAL, "rv_stitch_open: n_chunks=%d is negative", n_chunks);
  if (L < 1 || L > h->cfg.max_output_len) return fail(h, RV_EINVAL, "max_output_len=%d outside [1,%d]", L, h->cfg.max_output_len);
  if (L - 1 > ST_LANES) return fail(h, RV_EUNSUPPORTED, "max_output_len %d exceeds %d", L, ST_LANES + 1);
  HIPCHK(h, hipSetDevice(h->cfg.device));
  RvStitchBuf* sb = new RvStitchBuf();
  sb->n = n_chunks; sb->L = L; sb->steps = L - 1;
  sb->win.assign((size_t)n_chunks * 5, -1);
  const size_t cells = std::max<size_t>((size_t)n_chunks * sb->steps, 1), rows = std::max<size_t>((size_t)n_chunks, 1);
  bool ok = hipMalloc((void**)&sb->bases, cells) == hipSuccess && hipMalloc((void**)&sb->probs, cells * 4) == hipSuccess &&
            hipMalloc((void**)&sb->lens, rows * 4) == hipSuccess;
  for (int i = 0; i < 4 && ok; ++i) ok = hipMalloc((void**)&sb->mv[i], cells * 4) == hipSuccess;
  // (rows that only a slab without steps, L == 1, writes: no letters)
  ok = ok && hipMemset(sb->lens, 0, rows * 4) == hipSuccess;
  if (!ok) { free_stitch_buf(sb); return fail(h, RV_ENOMEM, "rv_stitch_open: device tables of %d rows: %s", n_chunks, hipGetErrorString(hipGetLastError())); }
  h->stitch_bufs.push_back(sb);
  *sb_out = sb;
  return RV_OK;
}
int rv_stitch_close(rv_handle h, rv_stitch sb) {
  if (!h) return RV_EINVAL;
  RvStitchBuf* k = find_stitch_buf(h, sb);
  if (!k) return fail(h, RV_EINVAL, "rv_stitch_close: not a stitch buffer of this handle");
  if (k->tickets > 0) return fail(h, RV_ESTATE, "rv_stitch_close: %d uncollected ticket(s) write into this stitch buffer: collect them first", k->tickets);
  h->stitch_bufs.erase(std::find(h->stitch_bufs.begin(), h->stitch_bufs.end(), k));
  hipSetDevice(h->cfg.device);
  free_stitch_buf(k);
  return RV_OK;
}
int rv_beam_search_submit_windows_stitch(rv_handle h, const int32_t* win, int32_t B, int32_t T_r, int32_t T_e, int32_t W, int32_t L,
                                         const uint8_t* lut, rv_stitch sb, int32_t row0, int32_t* ticket) {
  if (!lut) return h ? fail(h, RV_EINVAL, "null lut") : RV_EINVAL;
  std::vector<RecWindow> rows; std::vector<int> ids; Call c;
  TRY(windows_call(h, win, B, T_r, T_e, W, L, rows, ids, c));
  RvStitchBuf* k = find_stitch_buf(h, sb);
  if (!k) return fail(h, RV_EINVAL, "rv_beam_search_submit_windows_stitch: not a stitch buffer of this handle");
  if (L != k->L) return fail(h, RV_EINVAL, "max_output_len=%d, but the stitch buffer was opened for %d", L, k->L);
  if (row0 < 0 || (long long)row0 + B > (long long)k->n)
    return fail(h, RV_EINVAL, "rows [%d,%lld) lie outside the stitch buffer's %d rows", row0, (long long)row0 + B, k->n);
  c.lut = lut; c.want_call_moves = true; c.stitch = k; c.stitch_row0 = row0;
  TRY(submit(h, c, ticket));
  hold_reads(h, *ticket, ids);
  h->stitch_tickets[*ticket] = k;
  k->tickets += 1;
  if (B > 0) memcpy(k->win.data() + (size_t)row0 * 5, win, sizeof(int32_t) * 5 * (size_t)B);
  return RV_OK;
}
int rv_beam_search_collect_stitch(rv_handle h, int32_t ticket, int32_t* S_out) {
  if (!h) return RV_EINVAL;
  return collect(h, ticket, nullptr, nullptr, nullptr, S_out, nullptr, nullptr, nullptr, true);
}
int rv_stitch_run(rv_handle h, rv_stitch sb, int32_t n_reads, const int32_t* read_rows, const RvStitchOut* out) {
  if (!h) return RV_EINVAL;
  RvStitchBuf* k = find_stitch_buf(h, sb);
  if (!k) return fail(h, RV_EINVAL, "rv_stitch_run: not a stitch buffer of this handle");
  if (k->tickets > 0) return fail(h, RV_ESTATE, "rv_stitch_run: %d uncollected ticket(s) write into this stitch buffer: collect them first", k->tickets);
  StIn d{k->bases, k->probs, k->lens, k->mv[0], k->mv[1], k->mv[2], k->mv[3], k->n, k->steps, 0};
  return stitch_core(h, d, k->win.data(), n_reads, read_rows, out, "rv_stitch_run");
}

// ---- forced alignment: the forced decode with its records kept, k_forced_moves behind the finalize
int rv_teacher_forced_moves(rv_handle h, const float* raw, const float* event, int32_t B, int32_t T_r, int32_t T_e, int32_t L,
                            const int32_t* targets, uint32_t omit_mask, int32_t* sample_id, float* logits, const RvScore* out,
                            const RvMoves* moves) {
  if (!h) return RV_EINVAL;
  if (moves_missing(moves, B, L)) return fail(h, RV_EINVAL, "null output pointer");
  const ForcedCall fc{targets, omit_mask, out};
  Call c = slab_call(raw, event, false, B, T_r, T_e, 1, L);
  c.greedy = true; c.tokens = sample_id; c.out2 = logits; c.forced = &fc; c.forced_moves = moves;
  int32_t S = 0;
  return run(h, c, &S);
}
int rv_teacher_forced_moves_dev(rv_handle h, const float* d_raw, const float* d_event, int32_t B, int32_t T_r, int32_t T_e, int32_t L,
                                const int32_t* d_targets, uint32_t omit_mask, int32_t* d_sample_id, float* d_logits, const RvScore* d_out,
                                const RvMoves* d_moves) {
  if (!h) return RV_EINVAL;
  if (moves_missing(d_moves, B, L)) return fail(h, RV_EINVAL, "null output pointer");
  const ForcedCall fc{d_targets, omit_mask, d_out};
  Call c = slab_call(d_raw, d_event, true, B, T_r, T_e, 1, L);
  c.greedy = true; c.tokens = d_sample_id; c.out2 = d_logits; c.forced = &fc; c.forced_moves = d_moves;
  int32_t S = 0;
  return run(h, c, &S);
}

int rv_beam_search_flush(rv_handle h) {
  if (!h) return RV_EINVAL;
  return flush_open_group(h);
}

int rv_set_option(rv_handle h, const char* key, int32_t value) {
  if (!h || !key) return RV_EINVAL;
  flush_open_group(h);               // a group still filling was submitted under the options as they were
  if (h->rnn == RV_RNN_BIGRU) TRY(refuse_gru_option(h, key, value));
  if (!strcmp(key, "group_inplace") && value != 0 && value != 1) return fail(h, RV_EINVAL, "group_inplace must be 0 or 1");
  if (!strcmp(key, "group_side_ev") && (value < -1 || value > 1)) return fail(h, RV_EINVAL, "group_side_ev must be -1 (where the hardware queues allow it), 0 or 1");
  if (!strcmp(key, "weight_parts")) {
    if (value != 1 && value != 2) return fail(h, RV_EINVAL, "weight_parts must be 2 (each weight as two f16 parts) or 1 (rounded to its first part)");
    if (uncollected(h)) return fail(h, RV_ESTATE, "collect the calls in flight before setting weight_parts");
  }
  if (!strcmp(key, "one_part_kernels") && value != 0 && value != 1) return fail(h, RV_EINVAL, "one_part_kernels must be 0 or 1");
  if (!strcmp(key, "fused_inproj")) {
    if (value < -1 || value > 1) return fail(h, RV_EINVAL, "fused_inproj must be 1 (always), 0 (never) or -1 (per call)");
    // an explicit 1 stands behind one kernel, the sixteen-chunk BiLSTM form: every other recurrence keeps its GEMM
    if (value == 1 && h->rnn == RV_RNN_BIGRU)
      return fail(h, RV_EUNSUPPORTED, "fused_inproj 1 is not served on a bigru handle: k_gru_rec_mx reads its layers' inputs from the split GEMM");
    if (value == 1 && h->opt.wide != 1 && h->opt.wide != -1)
      return fail(h, RV_EUNSUPPORTED, "fused_inproj 1 is not served with wide_recurrence %d: only the sixteen-chunk matrix-pipe recurrence projects its own "
                  "inputs (the %s keeps its projection)", h->opt.wide, h->opt.wide == 2 ? "eight-chunk form" : "packed-FMA path");
  }
  if (!strcmp(key, "wide_recurrence") && h->opt.fused_inproj == 1 && (value == 0 || value == 2))
    return fail(h, RV_EUNSUPPORTED, "wide_recurrence %d is not served with fused_inproj 1: only the sixteen-chunk matrix-pipe recurrence projects its own "
                "inputs; set fused_inproj to 0 or -1 first", value);
  if (!strcmp(key, "gru_persistent")) {
    if (value != 0 && value != 1) return fail(h, RV_EINVAL, "gru_persistent must be 0 or 1");
    if (h->rnn != RV_RNN_BIGRU)
      return fail(h, RV_EUNSUPPORTED, "gru_persistent is an option of a bigru handle: this one is bilstm, whose decode is persistent by default (option persistent_decode)");
    if (h->cfg.dec_depth != 1)
      return fail(h, RV_EUNSUPPORTED, "gru_persistent serves a bigru handle of one decoder cell: this one has decoder_depth %d, whose cells decode per step", h->cfg.dec_depth);
    if (uncollected(h)) return fail(h, RV_ESTATE, "collect the calls in flight before setting gru_persistent");
    // on: the images now, from the weights in force if there are any (else the next rv_load_weights builds them); off: nothing is freed
    if (value == 1 && h->loaded && !h->gimg.built) TRY(build_gru_persist(h, nullptr));
  }
  h->opt.gen++;                      // slab graphs captured under the old options are rebuilt on their next use
  if (!strcmp(key, "weight_parts")) h->opt.weight_parts = value;      // (in force from the next rv_load_weights)
  else if (!strcmp(key, "one_part_kernels")) h->opt.one_part = value;
  else if (!strcmp(key, "gru_persistent")) h->opt.gru_persist = value;
  else if (!strcmp(key, "debug_taps")) h->opt.taps = value != 0;
  else if (!strcmp(key, "slab_graph")) h->opt.slab_graph = value != 0;
  else if (!strcmp(key, "coalesce")) {
    if (value < -1 || value > RV_MAX_MEMBERS) return fail(h, RV_EINVAL, "coalesce must be -1 (chosen from async_depth), 0, 1 or 2..%d", RV_MAX_MEMBERS);
    h->opt.coalesce = value;
  }
  else if (!strcmp(key, "group_inplace")) h->opt.group_inplace = value;
  else if (!strcmp(key, "group_side_ev")) h->opt.group_side_ev = value;
  else if (!strcmp(key, "persist_taps")) h->opt.ptaps = value != 0;
  else if (!strcmp(key, "fused_memory")) h->opt.fused_mem = value != 0;
  else if (!strcmp(key, "fused_inproj")) h->opt.fused_inproj = value;
  else if (!strcmp(key, "use_graph")) h->opt.graph = value != 0;
  else if (!strcmp(key, "flash_attend")) h->opt.flash = value != 0;
  else if (!strcmp(key, "persistent_decode")) h->opt.persist = value != 0;
  else if (!strcmp(key, "concurrent_encoders")) h->opt.side_ev = value != 0;
  else if (!strcmp(key, "lane_projection")) h->opt.lane_inproj = value != 0;
  else if (!strcmp(key, "fused_projection")) h->opt.fuse = value != 0;
  else if (!strcmp(key, "tail_wave")) h->opt.tail_wave = value != 0;
  else if (!strcmp(key, "wide_recurrence")) h->opt.wide = value < 0 ? -1 : (value == 2 ? 2 : (value != 0));
  else if (!strcmp(key, "async_depth")) {
    if (value < 1 || value > RV_MAX_ASYNC) return fail(h, RV_EINVAL, "async_depth must be 1..%d", RV_MAX_ASYNC);
    h->opt.async_depth = value;
    // every context is one HIP stream; the runtime multiplexes a process's streams onto GPU_MAX_HW_QUEUES hardware queues (4 unless the
    // environment says otherwise when the runtime starts).  More contexts than queues: some share a queue and their slabs serialise.
    const char* q = nullptr;
    if (value > hw_queues(&q))
      return fail(h, RV_WQUEUES, "async_depth %d set, but GPU_MAX_HW_QUEUES is %s: contexts beyond the hardware queues share one and serialise "
                  "(C3: depth 10 -> 278 k chunks/s on 8 queues, 317 k on 16); set GPU_MAX_HW_QUEUES >= %d in the environment before the "
                  "process's first HIP call", value, q ? q : "unset (4 queues)", value);
  }
  else if (!strcmp(key, "matrix_attention")) h->opt.mx_att = value != 0;
  else if (!strcmp(key, "matrix_cell")) h->opt.mx_cell = value != 0;
  else if (!strcmp(key, "split_projection")) h->opt.split_proj = value < 0 ? 0 : (value > 2 ? 2 : value);
  else if (!strcmp(key, "attend_threads")) {
    if (value != 0 && value != 256 && value != 512) return fail(h, RV_EINVAL, "attend_threads must be 0, 256 or 512");
    h->opt.att_nt = value;
  }
  else if (!strcmp(key, "decode_split")) h->opt.split = value < 1 ? 1 : (value > 4 ? 4 : value);
  else if (!strcmp(key, "profile")) h->opt.profile = value < 0 ? 0 : (value > 3 ? 3 : value);
  else return fail(h, RV_EINVAL, "unknown option '%s'", key);
  return RV_OK;
}

int rv_get_tensor(rv_handle h, const char* name, float* dst, size_t dst_floats, size_t* n_written) {
  if (!h || !name || !n_written) return RV_EINVAL;
  SlabCtx* cx = h->slabs[0];            // slot 0's last call, and the handle's S
  const size_t B = cx->lB, W = cx->fact.lW, Tm = cx->lTm, S = h->lS, V = h->cfg.vocab;
  const void* src = nullptr; size_t n = 0; int kind = 0;   // 0 f32, 1 i32, 2 u8
  const DecState& d = cx->dec_st;
  if (!strcmp(name, "enc_output")) { src = cx->enc_out; n = B * Tm * RV_E; }
  else if (!strcmp(name, "mask")) { src = cx->mask; n = B * Tm; kind = 2; }
  else if (!strcmp(name, "keys")) {
    if (!cx->fact.lkeys) return fail(h, RV_ESTATE, "keys were not built by the last call (single-pass attend); set debug_taps=1");
    src = cx->keys; n = B * Tm * RV_U;
  }
  else if (!strcmp(name, "projected_memory")) {
    if (!cx->fact.lpersist) return fail(h, RV_ESTATE, "the projected memory is built for the persistent decode only (the last call ran the per-step kernels)");
    if (cx->fact.lmem2_stale) {   // the decode projected its chunks itself and stored nothing: the same product of that call's enc_out, now
      HIPCHK(h, hipSetDevice(h->cfg.device));
      launch_gemm_mem_split(cx->enc_out, (int)(B * Tm), h->rnn == RV_RNN_BIGRU ? h->gimg.gWmp16 : h->img.Wmp16, cx->mem2, cx->stream);
      HIPCHK(h, hipStreamSynchronize(cx->stream));
      cx->fact.lmem2_stale = 0;
    }
    src = cx->mem2; n = B * Tm * RV_E;
  }
  else if (!strcmp(name, "coalesce_stats")) {   // groups launched, slabs they held, members of the largest, slabs per group in force
    *n_written = 4;
    if (!dst || dst_floats < 4) return fail(h, RV_EINVAL, "coalesce_stats needs 4 floats");
    dst[0] = (float)h->co_groups; dst[1] = (float)h->co_slabs; dst[2] = (float)h->co_largest;
    dst[3] = (float)coalesce_n(h, async_depth(h));
    return RV_OK;
  }
  else if (!strcmp(name, "read_stats")) {       // device allocations made for reads, reads alive, puts, read slots (alive or kept for reuse), k_expand_windows launches
    *n_written = 5;
    if (!dst || dst_floats < 5) return fail(h, RV_EINVAL, "read_stats needs 5 floats");
    long long alive = 0;
    for (const Read& r : h->reads) alive += r.live ? 1 : 0;
    dst[0] = (float)h->read_allocs; dst[1] = (float)alive; dst[2] = (float)h->read_puts; dst[3] = (float)h->reads.size(); dst[4] = (float)h->win_expands;
    return RV_OK;
  }
  else if (!strcmp(name, "rec_stamps")) {
    if (!cx->rec_ts) return fail(h, RV_ESTATE, "set RV_REC_STAMPS=1 before rv_create (and load a -DRV_REC_STAMPS build)");
    long long ts[24];
    HIPCHK(h, hipMemcpy(ts, cx->rec_ts, sizeof ts, hipMemcpyDeviceToHost));
    *n_written = 24;
    if (!dst || dst_floats < 24) return fail(h, RV_EINVAL, "rec_stamps needs 24 floats");
    for (int i = 0; i < 24; ++i) dst[i] = (float)ts[i];
    return RV_OK;
  }
  else if (!strcmp(name, "kernel_forms") || !strcmp(name, "kernel_form_list") || !strcmp(name, "kernel_form_list_1p") || !strcmp(name, "kernel_form_list_proj") ||
           !strcmp(name, "group_kernel_forms")) {
    FormLog all;
    const FormLog* f = &cx->lforms;
    if (!strcmp(name, "kernel_form_list") && h->rnn == RV_RNN_BIGRU) {      // the list answers for the handle's family
      FormLog dec;
      list_gru_forms(all); list_decode_forms(dec); list_decode_forms_gru(all);
      for (int i = 0; i < dec.n; ++i)      // (the attend kernels; the persistent decode is k_dec_persist_gru's list)
        if (dec.row[i][0] != RV_K_DEC_PERSIST) all.add(dec.row[i][0], dec.row[i][1], dec.row[i][2], dec.row[i][3], dec.row[i][4]);
      f = &all;
    } else if (!strcmp(name, "kernel_form_list")) {
      list_rec_forms(all); list_mx_forms(all); list_decode_forms(all);
      f = &all;
    } else if (!strcmp(name, "kernel_form_list_1p")) {
      list_decode_forms_1p(all);
      f = &all;
    } else if (!strcmp(name, "kernel_form_list_proj")) {
      list_mx_proj_forms(all);
      f = &all;
    } else if (!strcmp(name, "group_kernel_forms")) {
      f = &h->gforms;
    } else if (!cx->lforms_ok) {
      return fail(h, RV_ESTATE, "kernel_forms: the last call replayed a slab graph (option slab_graph), which launches nothing on the host");
    }
    if (f->full) return fail(h, RV_EUNSUPPORTED, "%s: more than %d forms (raise RV_FORM_ROWS)", name, RV_FORM_ROWS);
    *n_written = (size_t)5 * f->n;
    if (*n_written && (!dst || dst_floats < *n_written)) return fail(h, RV_EINVAL, "%s needs %zu floats", name, *n_written);
    for (int i = 0; i < f->n; ++i)
      for (int j = 0; j < 5; ++j) dst[5 * i + j] = (float)f->row[i][j];
    return RV_OK;
  }
  else if (!strcmp(name, "dbg_stamps")) {
    if (!d.dbg_ts) return fail(h, RV_ESTATE, "set RV_DBG_STAMPS=1 before rv_create");
    long long ts[16];
    HIPCHK(h, hipMemcpy(ts, d.dbg_ts, sizeof ts, hipMemcpyDeviceToHost));
    *n_written = 16;
    if (!dst || dst_floats < 16) return fail(h, RV_EINVAL, "dbg_stamps needs 16 floats");
    for (int i = 0; i < 16; ++i) dst[i] = (float)(ts[i] - ts[0]);
    return RV_OK;
  }
  else if ((!strncmp(name, "step_", 5) || !strcmp(name, "parent_ids")) && cx->fact.lsplit > 1)
    return fail(h, RV_ESTATE, "per-step records are laid out per sub-slab when decode_split > 1; read them with decode_split=1 or debug_taps=1");
  else if (!strcmp(name, "chunk_steps")) {
    if (!cx->fact.lpersist) return fail(h, RV_ESTATE, "chunk_steps exist only after a persistent decode");
    src = cx->d_chunk_steps; n = B; kind = 1;
  }
  else if (!strcmp(name, "step_moves")) {
    if (!cx->lmoves || !cx->d_step_moves) return fail(h, RV_ESTATE, "step_moves are the records of a moves call (rv_beam_search_moves*): the last call on this context was none");
    src = cx->d_step_moves; n = S * B * W * RV_MOVE_COLS;
  }
  else if (!strcmp(name, "step_ids")) { src = d.step_ids; n = S * B * W; kind = 1; }
  else if (!strcmp(name, "parent_ids")) { src = d.parent_ids; n = S * B * W; kind = 1; }
  else if (!strcmp(name, "step_scores")) { src = d.step_scores; n = S * B * W; }
  else if (!strcmp(name, "step_logits")) {
    if (!cx->ltaps && !cx->lgreedy && !cx->lptaps) return fail(h, RV_ESTATE, "step_logits needs option debug_taps=1 or persist_taps=1");
    src = d.step_logits; n = S * B * W * V;
  } else if (!strcmp(name, "step_alignments")) {
    if (cx->ltaps) src = cx->step_align;
    else if (cx->lptaps && cx->fact.lpersist) src = cx->palign;   // [S][B][W][T_m] as the per-step tap
    else return fail(h, RV_ESTATE, "step_alignments needs option debug_taps=1, or persist_taps=1 on the persistent decode");
    n = S * B * W * Tm;
  } else return fail(h, RV_EINVAL, "unknown tensor '%s'", name);
  *n_written = n;
  if (n == 0) return RV_OK;
  if (!dst || dst_floats < n) return fail(h, RV_EINVAL, "tensor '%s' needs %zu floats, buffer holds %zu", name, n, dst_floats);
  HIPCHK(h, hipSetDevice(h->cfg.device));
  if (kind == 0) {
    HIPCHK(h, hipMemcpy(dst, src, n * sizeof(float), hipMemcpyDeviceToHost));
    if (src == cx->step_align && cx->fact.lflash && !cx->lmoves) {      // (a moves call's tap is the two-pass launch's: alignments already)
      // the single-pass kernel taps raw log2-domain masked scores; normalise here (debug path only)
      for (size_t r = 0; r < n / Tm; ++r) {
        float* a = dst + r * Tm;
        double mx = -INFINITY, sum = 0;
        for (size_t t = 0; t < Tm; ++t) mx = std::max(mx, (double)a[t]);
        for (size_t t = 0; t < Tm; ++t) sum += std::exp2((double)a[t] - mx);
        for (size_t t = 0; t < Tm; ++t) a[t] = (float)(std::exp2((double)a[t] - mx) / sum);
      }
    }
  } else if (kind == 1) {
    std::vector<int32_t> tmp(n);
    HIPCHK(h, hipMemcpy(tmp.data(), src, n * sizeof(int32_t), hipMemcpyDeviceToHost));
    for (size_t i = 0; i < n; ++i) dst[i] = (float)tmp[i];
  } else {
    std::vector<uint8_t> tmp(n);
    HIPCHK(h, hipMemcpy(tmp.data(), src, n, hipMemcpyDeviceToHost));
    for (size_t i = 0; i < n; ++i) dst[i] = (float)tmp[i];
  }
  return RV_OK;
}

int rv_get_profile(rv_handle h, const char* kernel, double* total_ms, int64_t* launches) {
  if (!h || !kernel || !total_ms || !launches) return RV_EINVAL;
  auto it = h->prof.find(kernel);
  if (it == h->prof.end()) { *total_ms = 0; *launches = 0; return RV_OK; }
  *total_ms = it->second.ms; *launches = it->second.n;
  return RV_OK;
}

int rv_profile_names(rv_handle h, char* dst, size_t dst_bytes) {
  if (!h || !dst || dst_bytes == 0) return RV_EINVAL;
  std::string s;
  for (auto& kv : h->prof) { if (!s.empty()) s += ';'; s += kv.first; }
  if (s.size() + 1 > dst_bytes) return fail(h, RV_EINVAL, "name buffer too small (%zu needed)", s.size() + 1);
  memcpy(dst, s.c_str(), s.size() + 1);
  return RV_OK;
}

int rv_reset_profile(rv_handle h) {
  if (!h) return RV_EINVAL;
  h->prof.clear();
  return RV_OK;
}

}  // extern "C"
