/* iyokan_hip.h — C ABI of the MI355X gate-bootstrapping backend (libiyokan_hip.so).
 *
 * This is the library boundary that replaces the cuFHE C++ API used by Iyokan's GPU worker
 * (/root/reference/src/iyokan_cufhe.{hpp,cpp}, /root/reference/src/tfhepp_cufhe_wrapper.hpp).
 * Each entry point cites the reference call it replaces.  Plain C types only: pointers,
 * sizes, ints.  No function throws or aborts (host allocation failure is IYK_ERR_NOMEM); every function returns an int status
 * (IYK_OK == 0, negative on error) and iyk_hip_last_error() describes the last failure on
 * the calling thread.  The reference ignores cuFHE's return values and dies via
 * error::die() -> exit(1) (/root/reference/src/error.hpp:22-48); the C++ adapter
 * (iyokan_amd/host/iyokan_hip.hpp) maps non-zero status to the same behaviour.
 *
 * Threading contract (= the reference's): all enqueue / query calls for one
 * stream come from one host thread at a time; enqueue and query never block.
 *
 * Data layouts
 *   TLWE lvl0 ciphertext  u32[n+1], mask a[0..n-1] then body b   (TFHEpp::TLWE<lvl0param>)
 *   ciphertext arena      u32[slots][n+1] in device memory; gates address slots by index
 *   bootstrapping key in  u32[n][(k+1)l][k+1][N]  torus domain   (EvalKey::getbk<lvl01param>,
 *                         required by the GPU path: /root/reference/src/iyokan_cufhe.cpp:734)
 *   key-switching key in  u32[kN][t][2^basebit-1][n+1]           (EvalKey::getiksk<lvl10param>)
 */
#ifndef IYOKAN_HIP_H
#define IYOKAN_HIP_H

#include <stdint.h>

#include "iyokan_hip_params.h"

#ifdef __cplusplus
extern "C" {
#endif

#define IYK_OK 0
#define IYK_ERR_INVALID (-1)   /* bad argument / unsupported parameter set */
#define IYK_ERR_STATE (-2)     /* not initialised, already initialised, stale handle */
#define IYK_ERR_HIP (-3)       /* a HIP runtime call failed (message in iyk_hip_last_error) */
#define IYK_ERR_NOMEM (-4)

/* Gate kinds.  Names follow Iyokan's gate tasks (DEFINE_TASK_GATE,
 * /root/reference/src/iyokan_cufhe.hpp:249-261): ANDNOT = a & ~b (cufhe::AndYN),
 * ORNOT = a | ~b (cufhe::OrYN), MUX(in0 = A, in1 = B, in2 = S) = S ? B : A
 * (cufhe::Mux(out, S, B, A)).  COPY is TaskCUFHEGateWIRE's host copy (:168-183). */
typedef enum iyk_gate_op {
    IYK_OP_AND = 0,
    IYK_OP_NAND = 1,
    IYK_OP_ANDNOT = 2,
    IYK_OP_OR = 3,
    IYK_OP_NOR = 4,
    IYK_OP_ORNOT = 5,
    IYK_OP_XOR = 6,
    IYK_OP_XNOR = 7,
    IYK_OP_MUX = 8,
    IYK_OP_NOT = 9,
    IYK_OP_CONSTONE = 10,
    IYK_OP_CONSTZERO = 11,
    IYK_OP_COPY = 12,
    IYK_OP__COUNT = 13
} iyk_gate_op;

typedef struct iyk_hip_stream iyk_hip_stream; /* opaque; replaces cufhe::Stream */

/* ---- library lifetime ------------------------------------------------------------------ */

/* Replaces cufhe::SetGPUNum(n) + cufhe::Initialize(ek)
 * (/root/reference/src/iyokan_cufhe.cpp:530-536, /root/reference/src/test0.cpp:679).
 * device_ids[ngpu] are HIP ordinals (NULL = 0..ngpu-1).  On every listed GPU: uploads the
 * torus-domain BK, forward-NTTs all n*(k+1)l*(k+1) polynomials on the device, uploads the
 * KSK (row-padded) and the twiddle tables.  Host buffers may be freed on return.
 * Requirements: N == 1024, k == 1, l*Bgbit <= 31, n <= 1023. */
int iyk_hip_init(int ngpu, const int* device_ids, const iyk_params* params,
                 const uint32_t* bk_torus, const uint32_t* ksk);

/* Replaces cufhe::CleanUp() (/root/reference/src/iyokan_cufhe.cpp:721).  All streams must
 * have been destroyed. */
int iyk_hip_cleanup(void);

int iyk_hip_is_initialized(void);
int iyk_hip_num_gpus(void);
int iyk_hip_get_params(iyk_params* out);
const char* iyk_hip_last_error(void);

/* ---- streams --------------------------------------------------------------------------- */

/* Replaces cufhe::Stream::Create() (/root/reference/src/iyokan_cufhe.hpp:13-16): a
 * non-blocking stream on GPU gpu_index (0 <= gpu_index < ngpu; the reference round-robins
 * streams over GPUs — pass `worker_index % ngpu` to reproduce that). */
int iyk_hip_stream_create(int gpu_index, iyk_hip_stream** out);

/* Adopt an existing hipStream_t (e.g. the one torch.distributed / RCCL work is ordered on)
 * instead of creating one; the caller keeps ownership of hip_stream.  Everything enqueued through an adopted stream — including
 * iyk_hip_gate_host, which for such a stream never parks the gate in a coalesced batch and never goes through the pinned mirror: its
 * result is copied device-to-host straight into `out`, ordered on hip_stream — is complete once hip_stream itself is
 * (hipStreamSynchronize, a hipEvent, a torch stream): no library-side poll is needed to see it. */
int iyk_hip_stream_wrap(int gpu_index, void* hip_stream, iyk_hip_stream** out);

/* Replaces cufhe::Stream::Destroy() (/root/reference/src/iyokan_cufhe.hpp:18-21). */
int iyk_hip_stream_destroy(iyk_hip_stream* st);

/* Replaces cufhe::StreamQuery(st) (/root/reference/src/iyokan_cufhe.hpp:196,236): 1 = all
 * work enqueued so far has finished, 0 = still running, < 0 = error.  Never blocks. */
int iyk_hip_stream_query(iyk_hip_stream* st);

/* GPU index (0 .. ngpu-1) the stream was created on. */
int iyk_hip_stream_gpu(iyk_hip_stream* st);

/* Blocks until the stream is idle (the reference spins on StreamQuery instead:
 * /root/reference/src/iyokan_cufhe.hpp:723-735). */
int iyk_hip_stream_sync(iyk_hip_stream* st);

/* ---- device-resident ciphertext arena -------------------------------------------------- */

/* Every call that takes an arena pointer also takes `arena_slots`, the number of ciphertexts the buffer
 * holds: all slot indices are validated against it and a bad descriptor is IYK_ERR_INVALID, never an
 * out-of-bounds device access. */

/* Device buffer of `slots` TLWE lvl0 ciphertexts on GPU gpu_index.  Replaces the
 * per-device mirror behind cufhe::Ctxt<lvl0param> (/root/reference/src/tfhepp_cufhe_wrapper.hpp:43-66);
 * a caller that already owns device memory (a torch tensor) may pass its pointer to the
 * batch calls directly instead. */
int iyk_hip_arena_alloc(int gpu_index, uint64_t slots, uint32_t** d_arena_out);
int iyk_hip_arena_free(int gpu_index, uint32_t* d_arena);

/* Host <-> arena copies of a CONTIGUOUS slot range, ordered on the stream (Ctxt::tlwehost <-> device;
 * /root/reference/src/iyokan_cufhe.hpp:217-222,238-241).  The host buffer must stay valid until the
 * stream is idle. */
int iyk_hip_arena_upload(iyk_hip_stream* st, uint32_t* d_arena, uint64_t arena_slots, uint64_t first_slot,
                         uint64_t count, const uint32_t* host_tlwe);
int iyk_hip_arena_download(iyk_hip_stream* st, const uint32_t* d_arena, uint64_t arena_slots,
                           uint64_t first_slot, uint64_t count, uint32_t* host_tlwe);

/* The same for a LIST of slots: host row j <-> arena slot slots[j].  One transfer + one scatter / gather
 * kernel for all the INPUT / OUTPUT / RAM cells of a network instead of one synchronous 2.5 KB copy per
 * cell (TaskCUFHEGateMem::set/get, /root/reference/src/iyokan_cufhe.hpp:80-88, copies per ciphertext).
 * upload_slots copies the host rows before returning; download_slots' host buffer must stay valid until
 * the stream is idle. */
int iyk_hip_arena_upload_slots(iyk_hip_stream* st, uint32_t* d_arena, uint64_t arena_slots, uint64_t count,
                               const int32_t* slots, const uint32_t* host_tlwe);
int iyk_hip_arena_download_slots(iyk_hip_stream* st, const uint32_t* d_arena, uint64_t arena_slots,
                                 uint64_t count, const int32_t* slots, uint32_t* host_tlwe);

/* Device -> device copy of a slot range (same or another GPU), ordered on `st`: growing an arena, the
 * DFF latch of a whole register file. */
int iyk_hip_arena_copy(iyk_hip_stream* st, uint32_t* d_dst, uint64_t dst_slots, uint64_t dst_first,
                       const uint32_t* d_src, uint64_t src_slots, uint64_t src_first, uint64_t count);

/* In-process multi-GPU (cufhe::SetGPUNum shape: streams of several GPUs driven by one host thread,
 * /root/reference/src/main.cpp:147-148): copy the listed slots of the arena replica on st_src's GPU to the
 * SAME slots of the replica on st_dst's GPU — gather on the source stream, one peer copy over xGMI and a
 * scatter on the destination stream, ordered by events (no host synchronisation).  This is the exchange of a
 * frontier's outputs at a level boundary; the reference bounces every ciphertext through host memory. */
int iyk_hip_arena_sync_slots(iyk_hip_stream* st_src, const uint32_t* d_src, uint64_t src_slots,
                             iyk_hip_stream* st_dst, uint32_t* d_dst, uint64_t dst_slots, uint64_t count,
                             const int32_t* slots);

/* The same exchange with ONE gather on the source and ndst destinations (the level boundary of an in-process multi-GPU
 * run: every other replica needs the rows this GPU produced).  Destination streams must be distinct and differ from
 * st_src.  Copies between different devices are hipMemcpyPeerAsync: direct over xGMI where iyk_hip_init enabled peer
 * access (iyk_hip_peer_access), staged through host memory by the runtime otherwise — same result either way. */
int iyk_hip_arena_sync_slots_multi(iyk_hip_stream* st_src, const uint32_t* d_src, uint64_t src_slots, int ndst,
                                   iyk_hip_stream* const* st_dst, uint32_t* const* d_dst, const uint64_t* dst_slots,
                                   uint64_t count, const int32_t* slots);

/* 1: GPU gpu_a reads GPU gpu_b's memory directly (hipDeviceEnablePeerAccess succeeded in iyk_hip_init, or same device);
 * 0: copies between them go through host memory; < 0: error.  Indices are positions in iyk_hip_init's device list. */
int iyk_hip_peer_access(int gpu_a, int gpu_b);

/* TRLWE lvl1 buffers (a(X) then b(X), 2N words each) for the CMUX-memory tasks: replaces
 * cufhe::cuFHETRLWElvl1 (/root/reference/src/iyokan_cufhe.hpp:592-661).  upload / download move a
 * contiguous range; the host side holds TFHEpp::TRLWE<lvl1param> in the same word order. */
int iyk_hip_trlwe_alloc(int gpu_index, uint64_t count, uint32_t** d_trlwe_out);
int iyk_hip_trlwe_free(int gpu_index, uint32_t* d_trlwe);
int iyk_hip_trlwe_upload(iyk_hip_stream* st, uint32_t* d_trlwe, uint64_t trlwe_slots, uint64_t first,
                         uint64_t count, const uint32_t* host_trlwe);
int iyk_hip_trlwe_download(iyk_hip_stream* st, const uint32_t* d_trlwe, uint64_t trlwe_slots, uint64_t first,
                           uint64_t count, uint32_t* host_trlwe);

/* Page-locked host memory for callers that stage whole batches themselves (iyk_hip_arena_upload / _download with a pageable
 * buffer work but are synchronous in effect: the runtime stages pageable memory itself and the device-to-host direction waits
 * for the stream).  cuFHE's Ctxt allocates its host side the same way.  No GPU index: page-locked memory is visible to all. */
int iyk_hip_host_alloc(uint64_t bytes, void** out);
int iyk_hip_host_free(void* p);

/* ---- the hot path ---------------------------------------------------------------------- */

/* Evaluate `count` mutually independent gates on arena slots, asynchronously on `st`.
 * Replaces `count` calls of cufhe::And/Nand/.../Mux/Not<lvl0param>(out, in.., st)
 * (/root/reference/src/iyokan_cufhe.hpp:249-261) with ONE batched launch sequence:
 *   linear step -> blind rotation (n CMUX external products, exact N-point negacyclic NTT, see
 *   iyk_hip_ntt_path) -> sample-extract(0) -> identity key-switch.
 * ops/in0/in1/in2/out are HOST arrays of length count (copied before return); in1/in2 are
 * ignored where the gate has fewer inputs (use -1).  A gate may write its output over one of its
 * OWN inputs; no output slot may be an input of ANOTHER gate of the same batch (the gates are
 * independent by contract).  Every index must lie in [0, arena_slots): anything else is IYK_ERR_INVALID.
 * With the environment variable IYK_HIP_DEBUG=1 at iyk_hip_init the independence contract itself is
 * verified (duplicate outputs, a gate reading another gate's output) and violations are IYK_ERR_INVALID.
 * Results are bit-identical to the CPU restatement in oracle/. */
int iyk_hip_gate_batch(iyk_hip_stream* st, uint32_t* d_arena, uint64_t arena_slots, uint64_t count,
                       const int32_t* ops, const int32_t* in0, const int32_t* in1, const int32_t* in2,
                       const int32_t* out);

/* The same gates on `lanes` copies of one circuit's arena image at once: K request packets of one circuit under one evaluation
 * key.  Lane r is the slots [r * lane_stride, (r + 1) * lane_stride) of the arena; the descriptors are those of ONE lane, every
 * index in [0, lane_stride), and stand for gate g of every lane, each lane at its own offset.  One lane's job lists are staged,
 * a kernel writes the lists of all lanes on the device (csrc/lane_jobs.hpp), and the launches of
 * iyk_hip_gate_batch run them as ONE batch of count * lanes gates: the kernels and launch shapes a flat batch of that many gates gets,
 * the same words per lane as iyk_hip_gate_batch on that lane alone.  Lanes cannot touch each other: every index a lane's gates read
 * or write lies in the lane's own slots.  Slots of a lane that no gate writes, and slots behind the last lane, are not touched.
 * Checked before anything is staged (IYK_ERR_INVALID, nothing enqueued): everything iyk_hip_gate_batch checks, with lane_stride in
 * the place of arena_slots; lanes and lane_stride not 0; lanes * lane_stride <= arena_slots and <= 2^31; count * lanes <= 2^30;
 * at most 2^31 - 1 rotations.  IYK_HIP_DEBUG=1 verifies the independence contract on one lane, which is every lane's.
 * lanes == 1 enqueues exactly what iyk_hip_gate_batch enqueues. */
int iyk_hip_gate_batch_lanes(iyk_hip_stream* st, uint32_t* d_arena, uint64_t arena_slots, uint64_t count,
                             const int32_t* ops, const int32_t* in0, const int32_t* in1, const int32_t* in2,
                             const int32_t* out, uint64_t lanes, uint64_t lane_stride);

/* One gate on HOST ciphertexts, same shape as cufhe::Nand(out, in0, in1, st): H2D of the
 * inputs, kernels, D2H of the result, all ordered on `st`; poll with iyk_hip_stream_query.
 * The inputs are copied before the call returns.  `out` must stay valid until the stream is idle and is WRITTEN when
 * iyk_hip_stream_query first returns 1 for the stream (or iyk_hip_stream_sync returns): the transfers go through a pinned
 * mirror inside the stream, so that neither the call nor the poll ever waits for the gate — the ciphertexts themselves may be
 * ordinary memory (TFHEpp::TLWE in a std::shared_ptr, as upstream's tasks hold them).  One gate in flight per stream
 * (the reference's shape: one Ctxt set per worker, /root/reference/src/iyokan_cufhe.hpp:290-312); a second call before the
 * first was seen idle finishes the first one first.
 *
 * COALESCING (default; IYK_HIP_COALESCE=0 at iyk_hip_init turns it off).  The reference relies on the GPU running the kernels of
 * its 240 - 800 one-gate streams side by side; this part runs launches of different streams of a process about four at a time
 * (hardware queues), i.e. ~1.5 k gates/s however many streams there are.  So the call does not launch: the gate is parked — its
 * operands copied into a page-locked batch buffer of the GPU — and ALL parked gates of the GPU go out as one iyk_hip_gate_batch on
 * a stream of the library's own at the second iyk_hip_stream_query of any parked stream (the reference's worker polls once right
 * after starting a gate, /root/reference/src/iyokan.hpp:851-874: the second poll means every worker of the sweep has handed its
 * gate in), at IYK_HIP_COALESCE_MAX parked gates (default 2048), or at iyk_hip_stream_sync.  iyk_hip_stream_query(st) returns 1
 * once st's gate has come back and `out` is written.  Results are the same words either way; the reference's harness shape
 * (one host thread, processAllGates(net, 240)) reaches ~60 % of the batched flavour's rate instead of ~1 %
 * (profiles/r05_per_gate.txt).  Other work enqueued on `st` is not ordered against a parked gate: a stream used for
 * iyk_hip_gate_host should be used for nothing else until it has been seen idle (the reference's workers do exactly that).
 * `out` belongs to the library from the call until the stream is seen idle and may be written EARLIER than that poll (when
 * another stream's iyk_hip_stream_sync has to drain the batch that holds this gate).  Threads: a stream is used by one host
 * thread at a time; different streams — of the same GPU too — may be driven from different threads (the parked gates of a GPU
 * are shared state behind one lock per GPU, never held across a blocking wait: a thread draining a batch does not stall the polls
 * of the others).  Destroying a stream with a parked gate completes the gate first.  Errors: a batch that fails on the GPU after
 * its gates were launched is reported by iyk_hip_stream_query / _sync of EVERY stream that had a gate in it (never a silent,
 * unwritten `out`), and the GPU's coalescer accepts no further batch (HIP errors of that kind are sticky).  Streams adopted with
 * iyk_hip_stream_wrap are exempt from all of this paragraph (see there). */
int iyk_hip_gate_host(iyk_hip_stream* st, int op, const uint32_t* in0, const uint32_t* in1,
                      const uint32_t* in2, uint32_t* out);

/* ---- measurement / test hooks ---------------------------------------------------------- */

/* Blind rotation + sample-extract only (cufhe::GateBootstrappingTLWE2TRLWElvl01NTT shape,
 * /root/reference/src/iyokan_cufhe.hpp:634-635, but extracted at index 0): for each job
 * lin = sa*arena[ia] + sb*arena[ib] + (0,..,0,off) -> TLWE lvl1 u32[N+1] at d_tlwe1 + job*(N+1).
 * Host arrays of length count; ib may be -1. */
int iyk_hip_blind_rotate_batch(iyk_hip_stream* st, const uint32_t* d_arena, uint64_t arena_slots,
                               uint64_t count, const int32_t* ia, const int32_t* ib, const int32_t* sa,
                               const int32_t* sb, const uint32_t* off, uint32_t* d_tlwe1);

/* Blind rotation only, result left as a TRLWE lvl1 (a(X) then b(X), 2N words) in row trlwe_out[job] of
 * d_trlwe (row `job` when trlwe_out is NULL).  Replaces cufhe::GateBootstrappingTLWE2TRLWElvl01NTT(
 * cuFHETRLWElvl1&, Ctxt&, st) (/root/reference/src/iyokan_cufhe.hpp:634-635: TaskCUFHERAMGateBootstrapping
 * writes the RAM cell's TRLWE `mem_`).  Same job description as iyk_hip_blind_rotate_batch. */
int iyk_hip_bootstrap_trlwe_batch(iyk_hip_stream* st, const uint32_t* d_arena, uint64_t arena_slots,
                                  uint64_t count, const int32_t* ia, const int32_t* ib, const int32_t* sa,
                                  const int32_t* sb, const uint32_t* off, uint32_t* d_trlwe,
                                  uint64_t trlwe_slots, const int32_t* trlwe_out);

/* Sample-extract(index 0) + identity key switch of TRLWEs into arena slots.  Replaces
 * cufhe::SampleExtractAndKeySwitch(Ctxt&, cuFHETRLWElvl1&, st) (/root/reference/src/iyokan_cufhe.hpp:601).
 * trlwe_index[g] selects the TRLWE (2N words each) in d_trlwe, out_slot[g] the destination slot. */
int iyk_hip_sample_extract_keyswitch_batch(iyk_hip_stream* st, const uint32_t* d_trlwe, uint64_t trlwe_slots,
                                           uint64_t count, const int32_t* trlwe_index, const int32_t* out_slot,
                                           uint32_t* d_arena, uint64_t arena_slots);

/* Sample-extract at coefficient index coeff_index[g] in [0, N) + identity key switch: the same with TFHEpp's
 * SampleExtractIndex<Lvl1>(res, trlwe, index) in front (TaskTFHEppSEI, /root/reference/src/iyokan_tfhepp.hpp:340-352: one output
 * bit of a ROM / RAM word per task).  a'[j] = a[h - j] for j <= h, -a[N + h - j] for j > h, b' = b[h]; index 0 gives the words of
 * iyk_hip_sample_extract_keyswitch_batch. */
int iyk_hip_sample_extract_index_keyswitch_batch(iyk_hip_stream* st, const uint32_t* d_trlwe, uint64_t trlwe_slots,
                                                 uint64_t count, const int32_t* trlwe_index, const int32_t* coeff_index,
                                                 const int32_t* out_slot, uint32_t* d_arena, uint64_t arena_slots);

/* ---- CMUX memories (ROM / RAM): the CMUX tree over TRLWE rows on the GPU --------------------------------------------------
 * Available on the default (FFT) path; after IYK_HIP_NTT=fp / goldilocks at init the trgsw_* and cmux calls return IYK_ERR_STATE.
 *
 * TRGSW lvl1 selector store in spectrum form: one slot = one step of the bootstrapping key's spectra,
 * (k+1) l * (k+1) * 2 * 512 * 16 bytes (192 KiB at the 128-bit set, 128 KiB at the 80-bit set).  Holds what TFHEpp keeps as
 * TRGSWFFT<lvl1param> (the TRGSWLvl1FFT inputs of TaskTFHEppROMUX / RAMUX, /root/reference/src/iyokan_tfhepp.hpp:238-240). */
int iyk_hip_trgsw_alloc(int gpu_index, uint64_t count, void** d_trgsw_out);
int iyk_hip_trgsw_free(int gpu_index, void* d_trgsw);
/* host rows are TFHEpp::TRGSW<lvl1param>: u32 [(k+1) l][k+1][N], torus domain (row c l + j = a TRLWE of zero plus
 * bit * 2^(32 - (j+1) Bgbit) at coefficient 0 of polynomial c).  Replaces TFHEpp::ApplyFFT2trgsw<lvl1param>.  The rows are copied
 * before return; the transform runs on st, ordered with the batches before and after it. */
int iyk_hip_trgsw_upload(iyk_hip_stream* st, void* d_trgsw, uint64_t trgsw_slots, uint64_t first, uint64_t count,
                         const uint32_t* host_trgsw);
/* `count` independent CMUXes on rows of a TRLWE store (iyk_hip_trlwe_*), asynchronous on st.  Job g:
 *     in1[g] >= 0:  T[out] = T[in0] + S[sel] [.] (T[in1] - T[in0])
 *                   replaces TFHEpp::CMUXFFT<Lvl1>(res, cs, c1, c0), res = c0 + cs [.] (c1 - c0), with c0 = T[in0], c1 = T[in1]:
 *                   a selector of 1 selects in1 (/root/reference/src/iyokan_tfhepp.hpp:267, 426-443, 627)
 *     in1[g] <  0:  T[out] = T[in0] + S[sel] [.] ((X^rot - 1) T[in0]),  rot[g] in [0, 2N)
 *                   replaces trgswfftExternalProduct after PolynomialMulByXaiMinusOne (/root/reference/src/iyokan_tfhepp.hpp:282-291)
 * [.] is the external product with the blind rotation's gadget, computed exactly mod 2^32 (TFHEpp's FFT product is not exact:
 * results agree after decryption, not word for word).  The five arrays are host arrays, copied before return.  A job may write
 * over its own inputs; no out[g] may be the in0 / in1 / out of ANOTHER job of the batch — checked on every call, as is every
 * index against the sizes stated: a violation is IYK_ERR_INVALID and nothing is launched. */
int iyk_hip_cmux_batch(iyk_hip_stream* st, const void* d_trgsw, uint64_t trgsw_slots, uint32_t* d_trlwe,
                       uint64_t trlwe_slots, uint64_t count, const int32_t* sel, const int32_t* in0,
                       const int32_t* in1, const int32_t* rot, const int32_t* out);
/* `count` independent CHAINS of CMUXes, asynchronous on st: the RAM write-back of one cell per job.  Job g, with S_j the selector
 * slot sel0[g] + j and j over 0 .. steps[g] - 1:
 *     acc = T[src]
 *     bit j of pattern[g] = 1:  acc = T[mem] + S_j [.] (acc - T[mem])      the cmux job (sel0 + j, in0 = mem, in1 = acc)
 *     bit j of pattern[g] = 0:  acc = acc    + S_j [.] (T[mem] - acc)      the cmux job (sel0 + j, in0 = acc, in1 = mem)
 *     T[out] = acc
 * so acc survives where selector j encrypts bit j of the pattern and T[mem] is chosen otherwise.  Replaces TaskTFHEppRAMCMUXs
 * (/root/reference/src/iyokan_tfhepp.hpp:622-628: *output_ = written, then CMUXFFT(*output_, normal or inverted selector j, *output_,
 * *mem_) per address bit, the NORMAL selector where bit j of the cell index is 1): pattern = the cell index, src = the written
 * TRLWE, mem = out = the cell; the reference's inverted selectors are this call's choice of in0 / in1.  One kernel, the accumulator
 * in LDS for all steps; word for word what steps[g] successive iyk_hip_cmux_batch jobs give (the product is exact).  The six arrays
 * are host arrays, copied before return.  Checked on every call, in O(count): 1 <= steps <= 32, sel0 >= 0 and sel0 + steps <=
 * trgsw_slots, every row < trlwe_slots, and no out[g] is the src / mem / out of ANOTHER job — a job may write over its own src or
 * mem, and jobs may share src (or mem).  A violation is IYK_ERR_INVALID and nothing is launched; IYK_ERR_STATE off the FFT path. */
int iyk_hip_cmux_chain_batch(iyk_hip_stream* st, const void* d_trgsw, uint64_t trgsw_slots, uint32_t* d_trlwe,
                             uint64_t trlwe_slots, uint64_t count, const int32_t* sel0, const int32_t* steps,
                             const uint32_t* pattern, const int32_t* src, const int32_t* mem, const int32_t* out);
/* `count` independent chains of ROTATE-form CMUXes, asynchronous on st: the lower half (LROMUX) of one ROM read per job.  Job g, with
 * (sel_j, rot_j) the entries first[g] + j of sel / rot, first[g] = steps[0] + .. + steps[g - 1] and j over 0 .. steps[g] - 1:
 *     acc = T[src]
 *     acc = acc + S[sel_j] [.] ((X^rot_j - 1) acc)                          the cmux job (sel_j, in0 = acc, in1 < 0, rot_j, out = acc)
 *     T[out] = acc
 * Replaces the loop of TaskTFHEppROMUX over the low address bits (/root/reference/src/iyokan_tfhepp.hpp:282-291: PolynomialMulByXaiMinusOne
 * of the accumulator by 2N - (N >> bit), trgswfftExternalProduct with that bit's selector, added to the accumulator): sel_j = the
 * selector of address bit log2(words per TRLWE) - bit, rot_j = 2N - (N >> bit), src = the row the upper tree left, out = the result
 * row.  One kernel, the accumulator in LDS for all steps, nothing read from the TRLWE store between them; word for word what
 * steps[g] successive iyk_hip_cmux_batch rotate jobs give (the product is exact).  sel and rot have sum(steps) entries, the jobs' steps
 * one after the other; the five arrays are host arrays, copied before return.  Checked on every call, in O(count + sum(steps)): 1 <=
 * steps <= 32, every sel in [0, trgsw_slots), every rot in [0, 2N), every row < trlwe_slots, and no out[g] is the src / out of ANOTHER
 * job — a job may write over its own src, and jobs may share src.  A violation is IYK_ERR_INVALID and nothing is staged or launched;
 * IYK_ERR_STATE off the FFT path.  With IYK_HIP_DEBUG=1 the kernel feeds iyk_hip_fft_round_error. */
int iyk_hip_cmux_rotate_chain_batch(iyk_hip_stream* st, const void* d_trgsw, uint64_t trgsw_slots, uint32_t* d_trlwe,
                                    uint64_t trlwe_slots, uint64_t count, const int32_t* steps, const int32_t* sel,
                                    const int32_t* rot, const int32_t* src, const int32_t* out);
/* `count` independent CMUX read trees, asynchronous on st: up to four levels of the upper half (UROMUX / RAMUX) of one memory read per
 * job.  Job g, with n = levels[g], halves the 2^n candidate rows T[first[g] .. first[g] + 2^n) n times:
 *     level b < n, i < 2^(n-1-b):   candidate i = candidate 2 i + S[sel0[g] + b] [.] (candidate 2 i + 1 - candidate 2 i)
 *     T[out] = the one candidate left
 * i.e. level b is the cmux jobs (sel0 + b, in0 = candidate 2 i, in1 = candidate 2 i + 1) of one iyk_hip_cmux_batch.  Replaces n
 * levels of the loops of TaskTFHEppROMUX's UROMUX and TaskTFHEppRAMUX (/root/reference/src/iyokan_tfhepp.hpp:262-271,425-443: CMUXFFT
 * over pairs of rows, one address bit per level; the RAM's loop keeps its results in place at a doubling stride, as this kernel does).  One kernel, one workgroup per job; the rows between the levels stay in the
 * workgroup's LDS and nothing but T[out] is written; word for word what levels[g] successive iyk_hip_cmux_batch launches give (the
 * product is exact).  The four arrays are host arrays, copied before return.  Checked on every call: 1 <= levels <= 4, selector slots
 * sel0 .. sel0 + levels - 1 in [0, trgsw_slots), the leaves and out in [0, trlwe_slots), and no out[g] is a leaf or the out of ANOTHER
 * job — a job may write over one of its own leaves, and jobs may share leaves.  A violation is IYK_ERR_INVALID and nothing is staged
 * or launched; IYK_ERR_STATE off the FFT path.  With IYK_HIP_DEBUG=1 the kernel feeds iyk_hip_fft_round_error. */
int iyk_hip_cmux_tree_batch(iyk_hip_stream* st, const void* d_trgsw, uint64_t trgsw_slots, uint32_t* d_trlwe, uint64_t trlwe_slots,
                            uint64_t count, const int32_t* sel0, const int32_t* levels, const int32_t* first, const int32_t* out);
/* The four CMUX batches above on `lanes` copies of one memory at once: K request packets of one circuit through one ROM / RAM clock.
 * Lane r's TRLWE rows are lane 0's + r * row_stride and its selector slots lane 0's + r * sel_stride (a rotate chain's steps: its sel
 * entries); the arrays are those of ONE lane and stand for job g of every lane.  One lane's list is staged, a kernel writes the lists
 * of all lanes on the device (csrc/cmux_lane_jobs.hpp, lane-major), and the UNCHANGED kernel of the parent call runs them as ONE
 * batch of count * lanes jobs, its grid taken from that total: the same words per lane as the parent call on that lane alone.
 * Checked before anything is staged (IYK_ERR_INVALID, nothing enqueued): everything the parent call checks, on lane 0's list against
 * the whole stores; lanes not 0, and no stride 0 with lanes > 1; count * lanes <= 2^24; the rows one lane's list reads or writes span
 * less than row_stride (max - min < row_stride), so no two lanes share a row; the highest row + (lanes - 1) * row_stride < trlwe_slots
 * and the highest selector slot + (lanes - 1) * sel_stride < trgsw_slots (selector slots are only read: lanes may interleave them);
 * no index of any lane reaches 2^31; for the rotate chain, sum(steps) * lanes <= 2^31 - 1.  lanes == 1 enqueues exactly what the
 * parent call enqueues and ignores the strides. */
int iyk_hip_cmux_batch_lanes(iyk_hip_stream* st, const void* d_trgsw, uint64_t trgsw_slots, uint32_t* d_trlwe, uint64_t trlwe_slots,
                             uint64_t count, const int32_t* sel, const int32_t* in0, const int32_t* in1, const int32_t* rot,
                             const int32_t* out, uint32_t lanes, uint64_t sel_stride, uint64_t row_stride);
int iyk_hip_cmux_chain_batch_lanes(iyk_hip_stream* st, const void* d_trgsw, uint64_t trgsw_slots, uint32_t* d_trlwe, uint64_t trlwe_slots,
                                   uint64_t count, const int32_t* sel0, const int32_t* steps, const uint32_t* pattern, const int32_t* src,
                                   const int32_t* mem, const int32_t* out, uint32_t lanes, uint64_t sel_stride, uint64_t row_stride);
int iyk_hip_cmux_rotate_chain_batch_lanes(iyk_hip_stream* st, const void* d_trgsw, uint64_t trgsw_slots, uint32_t* d_trlwe,
                                          uint64_t trlwe_slots, uint64_t count, const int32_t* steps, const int32_t* sel,
                                          const int32_t* rot, const int32_t* src, const int32_t* out, uint32_t lanes, uint64_t sel_stride,
                                          uint64_t row_stride);
int iyk_hip_cmux_tree_batch_lanes(iyk_hip_stream* st, const void* d_trgsw, uint64_t trgsw_slots, uint32_t* d_trlwe, uint64_t trlwe_slots,
                                  uint64_t count, const int32_t* sel0, const int32_t* levels, const int32_t* first, const int32_t* out,
                                  uint32_t lanes, uint64_t sel_stride, uint64_t row_stride);
/* T[out] = T[a] + T[b] mod 2^32 per job, with b0_offset added to coefficient 0 of the b polynomial; asynchronous on st, host
 * arrays copied before return.  The tail of TFHEpp::HomMUXwoSE<Lvl01> (TaskTFHEppGateMUXWoSE, /root/reference/src/iyokan_tfhepp.hpp:
 * 500-508): with a, b the rows of the two blind rotations iyk_hip_bootstrap_trlwe_batch(cs + c1 - mu) and (-cs + c0 - mu) and
 * b0_offset = mu, T[out] is the TRLWE of cs ? c1 : c0.  out[g] may be a[g] or b[g]; no out[g] may be the a / b / out of ANOTHER
 * job, every row < trlwe_slots: checked on every call, a violation is IYK_ERR_INVALID and nothing is launched.  Available on every
 * path. */
int iyk_hip_trlwe_add_batch(iyk_hip_stream* st, uint32_t* d_trlwe, uint64_t trlwe_slots, uint64_t count, const int32_t* a,
                            const int32_t* b, const int32_t* out, uint32_t b0_offset);

/* ---- private key switch: lvl2 TLWEs (64-bit torus) -> TRLWE rows -> TRGSW selector slots ----------------------------------------
 * The second half of circuit bootstrapping (TaskTFHEppCB / CBInv / CBWithInv, /root/reference/src/iyokan_tfhepp.hpp:194-236, 384-407,
 * in front of every ROMUX / RAMUX / RAMCMUXs port, :738-802): the server makes the selector slots of the CMUX memories from
 * ciphertexts instead of taking them from the holder of the secret key.  The first half (lvl0 -> lvl2 blind rotation) is
 * iyk_hip_cb_rotate_batch further down; it writes the lvl2 store below.  Integer only: available on every path, exact, order-free (sums mod 2^32).
 *
 * The key, one object per GPU: u32 [k+1][n_in+1][t][2^basebit - 1][k+1][N] — row K[c][i][j][u] is a lvl1 TRLWE (a(X), then b(X)) whose
 * phase b - a s1 is (u+1) 2^(32 - (j+1) basebit) sigma_i f_c(X) + noise, sigma_i = s2[i] (i < n_in), sigma_{n_in} = -1, f_1 = 1, f_0 = -s1(X)
 * (TFHEpp's PrivKeySwitchKey<lvl21param>: n_in = 2048, t = 10, basebit = 3, 2.35 GB).  n_in, t, basebit are run-time values of the key.
 * _create refuses (IYK_ERR_INVALID) n_in = 0, basebit outside 1..8, basebit * t > 63; an allocation failure is IYK_ERR_HIP, leaves no
 * state behind and touches no stream.  _upload copies rows [first_row, first_row + row_count) of the host layout before it returns
 * (so a caller never holds more than a window of the key) and orders the transfer on st.  _key_bytes: device bytes of the live keys of
 * one GPU. */
int iyk_hip_privks_key_create(int gpu_index, uint32_t n_in, uint32_t t, uint32_t basebit, void** out);
int iyk_hip_privks_key_upload(iyk_hip_stream* st, void* key, uint64_t first_row, uint64_t row_count, const uint32_t* host_rows);
int iyk_hip_privks_key_free(void* key);
int iyk_hip_privks_key_bytes(int gpu_index, uint64_t* out);
/* A window of a SEEDED key: the client sends a public 256-bit mask seed and the b polynomials only, u32 [row_count][N] (half the bytes
 * of _upload's window); the a polynomial of host row R is words 0 .. N - 1 of the ChaCha20 stream of (mask_seed, kind 1, R) — state
 * words 4 .. 11 the seed as little-endian u32, 12 the block index inside the row, 13 / 14 the row index low / high, 15 the kind
 * (csrc/key_expand.hpp) — and is written into the store by key_mask_expand_kernel on st, which also places the b halves.  host_b is
 * copied before return and goes through the same page-locked ring as _upload.  Seeded and unseeded windows may be mixed on one key;
 * the device-resident key is the same size either way.  Checked before anything is staged or launched: a null seed / key / buffer,
 * a window outside the key, an empty window, a stream of another replica or GPU than the key's are IYK_ERR_INVALID and leave the
 * store unchanged. */
int iyk_hip_privks_key_upload_seeded(iyk_hip_stream* st, void* key, const uint8_t* mask_seed /* [32] */, uint64_t first_row,
                                     uint64_t row_count, const uint32_t* host_b /* u32 [row_count][N] */);
/* TLWE lvl2 store: u64 [slots][n_in+1], a[0 .. n_in-1] then b (TFHEpp::TLWE<lvl2param>) — what the lvl0 -> lvl2 blind rotation will
 * write.  upload / download move a contiguous range, ordered on the stream; the host buffer must stay valid until the stream is idle. */
int iyk_hip_tlwe2_alloc(int gpu_index, uint32_t n_in, uint64_t slots, uint64_t** d_tlwe2_out);
int iyk_hip_tlwe2_free(int gpu_index, uint64_t* d_tlwe2);
int iyk_hip_tlwe2_upload(iyk_hip_stream* st, uint64_t* d_tlwe2, uint32_t n_in, uint64_t tlwe2_slots, uint64_t first, uint64_t count,
                         const uint64_t* host_tlwe2);
int iyk_hip_tlwe2_download(iyk_hip_stream* st, const uint64_t* d_tlwe2, uint32_t n_in, uint64_t tlwe2_slots, uint64_t first,
                           uint64_t count, uint64_t* host_tlwe2);
/* `count` independent key switches, asynchronous on st.  Job g, with w_i the words of TLWE in[g] of a store of the key's n_in,
 * wbar_i = w_i + 2^(63 - basebit t) and d_j(w) = (wbar >> (64 - (j+1) basebit)) & (2^basebit - 1):
 *     T[out[g]] = - sum_{i <= n_in} sum_{j < t, d_j(w_i) != 0} K[c[g]][i][j][d_j(w_i) - 1]      (mod 2^32, all 2N words)
 * a TRLWE of phase f_c (b - <a, s2>) / 2^32: from a lvl2 TLWE of bit * 2^(64 - (r+1) Bgbit), row c l + r of the bit's TRGSW as
 * iyk_hip_trgsw_upload takes it.  Replaces TFHEpp::PrivKeySwitch<lvl21param> inside CircuitBootstrappingFFT.  The i range of a job is
 * split over workgroups whose partial sums meet by integer atomics in a row zeroed first: word for word the same whatever the split.
 * The three arrays are host arrays, copied before return.  Checked on every call, in O(count): every index against the size stated,
 * c in [0, k], no two jobs with the same out — a violation is IYK_ERR_INVALID and nothing is launched. */
int iyk_hip_privks_batch(iyk_hip_stream* st, const void* key, const uint64_t* d_tlwe2, uint64_t tlwe2_slots, uint64_t count,
                         const int32_t* in, const int32_t* c, uint32_t* d_trlwe, uint64_t trlwe_slots, const int32_t* out);
/* The device-resident twin of iyk_hip_trgsw_upload: selector out_slot[g] is made by the same transform from the (k+1) l torus-domain
 * rows rows[g][0 .. (k+1) l - 1] of a TRLWE store, in row order c l + r (they are gathered into scratch of the stream first).
 * Asynchronous on st, host arrays copied before return.  A duplicate out_slot or an index outside its store is IYK_ERR_INVALID and
 * nothing is launched; IYK_ERR_STATE off the FFT path. */
int iyk_hip_trgsw_from_rows(iyk_hip_stream* st, void* d_trgsw, uint64_t trgsw_slots, uint64_t count, const int32_t* out_slot,
                            const uint32_t* d_trlwe, uint64_t trlwe_slots, const int32_t* rows /* [count][(k+1) l] */);

/* ---- circuit bootstrapping, first half: lvl0 -> lvl2 blind rotation (N2 = 2048, k = 1, 64-bit torus) -----------------------------
 * TFHEpp's GateBootstrappingTLWE2TLWEFFTvariableMu followed by + mu, once per gadget digit of an address bit, inside
 * CircuitBootstrappingFFT<lvl02param, lvl21param> (TaskTFHEppCB / CBInv / CBWithInv).  Job g = {in, sign, off, mu, out} on a lvl0 TLWE
 * store u32 [tlwe0_slots][key.n + 1] (the arena, when key.n is the initialised n) and a lvl2 store of n_in = 2048:
 *     lin = sign * W0[in] + (0, .., 0, off);  abar_i = (lin_i + 2^19) >> 20;  acc = X^(2 N2 - (lin_n >> 20)) * (0, mu (1 + .. + X^(N2-1)));
 *     acc += BK2_i [.] ((X^abar_i - 1) acc) for i < n;  W2[out] = SampleExtractIndex(acc, 0) + (0, .., 0, mu)
 * a lvl2 TLWE of 2 mu where the phase of lin is positive, of 0 where it is negative.  mu_r = 2^(63 - (r+1) Bgbit), r < l, gives the TLWEs
 * iyk_hip_privks_batch takes, slot order bit * l + r.  sign = -1: the reference's CircuitBootstrappingFFTInv.
 * Exact: every output word is the schoolbook negacyclic product mod 2^64 (integer field, key words split in two 32-bit halves: csrc/cb_rotate.hpp).
 * Integer only: available on every path.
 *
 * The key, one object per GPU: the torus-domain lvl2 TRGSW of every lvl0 key bit, u64 [n][(k+1) l2][k+1][N2] on the host (row c l2 + j:
 * a lvl2 TRLWE of zero plus s0[i] 2^(64 - (j+1) Bgbit2) at coefficient 0 of polynomial c), is uploaded in windows of steps through the
 * stream's page-locked ring and transformed on the stream into u64 [n][2 halves][(k+1) l2][k+1][N2] (333 MB at n = 636).  1 <= n <= 2047;
 * (l2, Bgbit2) = (4, 9) is the one instantiated pair, anything else is IYK_ERR_INVALID.  create allocates and does nothing else; a failed
 * allocation is IYK_ERR_HIP and leaves nothing behind.  upload: host words copied before return, asynchronous on st; the FIRST upload of
 * a key also sends the transform's tables (32 KiB) ahead of its window, so an upload on another stream must be ordered after it; a stream of another
 * replica than the key's is IYK_ERR_INVALID.  bytes: device bytes of the live keys of one GPU (0 again after iyk_hip_cleanup + iyk_hip_init;
 * a key of the earlier initialisation may still be freed and leaves the new count alone). */
int iyk_hip_bk2_key_create(int gpu_index, uint32_t n, uint32_t l2, uint32_t Bgbit2, void** out);
int iyk_hip_bk2_key_upload(iyk_hip_stream* st, void* key, uint64_t first_step, uint64_t step_count,
                           const uint64_t* host_trgsw /* u64 [step_count][(k+1) l2][k+1][N2], torus domain */);
int iyk_hip_bk2_key_free(void* key);
int iyk_hip_bk2_key_bytes(int gpu_index, uint64_t* out);
/* A window of a SEEDED lvl2 key, as iyk_hip_privks_key_upload_seeded: host_b holds the b polynomials only, the a polynomial of host row
 * R = step (k+1) l2 + r is a[m] = w[2m] | w[2m+1] << 32 of the ChaCha20 stream of (mask_seed, kind 2, R).  The window is staged as
 * _upload stages it, key_mask_expand_kernel fills the a polynomials of the staged torus-domain window, and the unchanged transform of
 * the key's form runs behind it; the first upload of a key, seeded or not, sends the tables.  Same checks, same refusals. */
int iyk_hip_bk2_key_upload_seeded(iyk_hip_stream* st, void* key, const uint8_t* mask_seed /* [32] */, uint64_t first_step,
                                  uint64_t step_count, const uint64_t* host_b /* u64 [step_count][(k+1) l2][N2] */);
/* count rotations, asynchronous on st, host arrays copied before return.  One workgroup per rotation; a batch wider than the GPU has
 * compute units runs in rounds inside the one launch.  Checked in O(count): every index inside its store, sign in {+1, -1}, no two jobs
 * with one out — a violation is IYK_ERR_INVALID and nothing is launched.  The kernel's time is what iyk_hip_last_batch_timing reports
 * (keyswitch_ms = 0). */
int iyk_hip_cb_rotate_batch(iyk_hip_stream* st, const void* key, const uint32_t* d_tlwe0, uint64_t tlwe0_slots, uint64_t count,
                            const int32_t* in, const int32_t* sign, const uint32_t* off, const uint64_t* mu, uint64_t* d_tlwe2,
                            uint64_t tlwe2_slots, const int32_t* out);
/* The many-digit form of the same rotation: ONE rotation per job gives the l lvl2 TLWEs of the constants mu[0 .. l) —
 * job g writes slots out[g] .. out[g] + l - 1, slot out[g] + r being a TLWE of 2 mu[r] where the phase of lin is positive and of 0 where
 * it is negative.  The mod switch is coarser by bw bits (2^bw >= l), the test vector interleaves the l constants, and coefficients
 * 0 .. l - 1 of the one accumulator are extracted; l = 1 gives iyk_hip_cb_rotate_batch's words.  mu: l words, shared by the batch.
 * Checked before anything is enqueued: 1 <= l <= 4, in / sign / off as above, out[g] + l inside the store, no two jobs' output ranges
 * overlapping, count <= 2^20 — a violation is IYK_ERR_INVALID and no store changes.  The form (iyk_hip_cb_rotate_form) is that of a
 * batch of `count` rotations: it does not depend on l. */
int iyk_hip_cb_rotate_many_batch(iyk_hip_stream* st, const void* key, const uint32_t* d_tlwe0, uint64_t tlwe0_slots, uint64_t count,
                                 const int32_t* in, const int32_t* sign, const uint32_t* off, uint32_t l, const uint64_t* mu,
                                 uint64_t* d_tlwe2, uint64_t tlwe2_slots, const int32_t* out);
/* *form_out = the kernel form a batch of count rotations would run on GPU gpu_index now: 0 = cb_rotate_kernel (256 lanes, the wide-batch
 * form), 1 = cb_rotate_lat_kernel (512 lanes, wave-owned polynomials, 4 barriers per step: the narrow-batch form).  Both give the same
 * words.  The answer of dispatch::cb_plan (csrc/dispatch.hpp) with the current environment: IYK_HIP_CB_KERNEL = wg / lat forces a form
 * and is read per batch; any other value is IYK_ERR_INVALID here and in every call that rotates (nothing is launched).  A GPU that did
 * not grant the narrow-batch form its 160 KiB of LDS at iyk_hip_init answers 0 whatever is asked for. */
int iyk_hip_cb_rotate_form(int gpu_index, uint64_t count, int* form_out);

/* The whole circuit bootstrapping of `bits` address bits as ONE checked call: the three calls above with the slot and row order of
 * cmux.selectors_from_tlwe0.  Bit b is TLWE in[b] of the lvl0 store, taken with sign[b] (-1: the selector of the negated bit); its l
 * rotations (mu_r = 2^(63 - (r+1) Bgbit), off = 0) go to lvl2 slots tlwe2_first + b l + r, its (k+1) l key switches to rows
 * (b (k+1) + c) l + r of the TRLWE scratch store, its selector to slot trgsw_first + b.  Checked before the first launch: everything the
 * three calls check, and what only their combination can — both keys and the stream of one replica, the lvl2 key's n = the initialised n
 * (the lvl0 store is the arena: rows of n + 1 words), the lvl2 store's n_in = 2048 = the
 * private key's n_in, bits * l lvl2 slots from tlwe2_first, at least bits (k+1) l scratch rows, bits selector slots from trgsw_first.  A
 * violation is IYK_ERR_INVALID (IYK_ERR_STATE off the FFT path): nothing is launched and no store changes.  The stream's selector scratch
 * and staging slot are grown to what the three calls need before the first launch as well.  Then the launches of
 * iyk_hip_cb_rotate_batch, iyk_hip_privks_batch and iyk_hip_trgsw_from_rows, in that order, asynchronous on st; host arrays are copied
 * before return. */
int iyk_hip_circuit_bootstrap_batch(iyk_hip_stream* st, const void* bk2_key, const void* privks_key, const uint32_t* d_tlwe0,
                                    uint64_t tlwe0_slots, const int32_t* in, const int32_t* sign, uint64_t* d_tlwe2, uint32_t tlwe2_n_in,
                                    uint64_t tlwe2_slots, uint64_t tlwe2_first, uint32_t* d_trlwe, uint64_t trlwe_slots, void* d_trgsw,
                                    uint64_t trgsw_slots, uint64_t trgsw_first, uint64_t bits);

/* iyk_hip_circuit_bootstrap_batch with the many-digit rotation: the same arguments, checks, slots, rows and selector meaning, `bits`
 * rotations instead of bits * l (the initialised l must be at most 4), then the unchanged iyk_hip_privks_batch and
 * iyk_hip_trgsw_from_rows.  The selectors' noise differs from the per-digit call's (other rotations), their plaintext does not. */
int iyk_hip_circuit_bootstrap_many_batch(iyk_hip_stream* st, const void* bk2_key, const void* privks_key, const uint32_t* d_tlwe0,
                                         uint64_t tlwe0_slots, const int32_t* in, const int32_t* sign, uint64_t* d_tlwe2,
                                         uint32_t tlwe2_n_in, uint64_t tlwe2_slots, uint64_t tlwe2_first, uint32_t* d_trlwe,
                                         uint64_t trlwe_slots, void* d_trgsw, uint64_t trgsw_slots, uint64_t trgsw_first, uint64_t bits);

/* Kernel-only time of the most recent iyk_hip_gate_batch on this stream, from HIP events
 * recorded on the stream around the blind-rotate and key-switch launches (milliseconds).
 * Blocks until those events have completed. */
int iyk_hip_last_batch_timing(iyk_hip_stream* st, float* blind_rotate_ms, float* keyswitch_ms);

/* Kernel-time log for a whole timed region (bench.py's roofline line): between _begin and
 * _end every iyk_hip_gate_batch on `st` records its own HIP events on the stream; _end
 * synchronises the stream and returns the number of batches and the summed blind-rotate /
 * key-switch kernel durations in milliseconds. */
int iyk_hip_timing_log_begin(iyk_hip_stream* st);
int iyk_hip_timing_log_end(iyk_hip_stream* st, uint64_t* batches, double* blind_rotate_ms,
                           double* keyswitch_ms);

/* Which exact-arithmetic field the blind rotation runs in: 1 = p = 3 * 2^48 + 1097729 on the FP64 FMA
 * pipe (default for both parameter sets; the 80-bit set splits its digits), 0 = 2^64 - 2^32 + 1 in 64-bit
 * integers (forced with the environment variable IYK_HIP_NTT=goldilocks at init, or chosen when a
 * parameter set does not meet the FP64 field's exactness bound).  Both give identical ciphertexts.
 *
 * A/B knobs for tests and measurements.  Read at every batch: IYK_HIP_ROT_KERNEL = fft / w32 / lat3 forces one
 * rotation kernel — fft: a wave per rotation, complex FFT, 8 points per lane (the default for full rounds); w32: a wave
 * per rotation on the FP64 field, 32 points per lane (the default for full rounds with IYK_HIP_NTT=fp); lat3: a workgroup
 * of 8 waves per rotation (the default for narrow frontiers).  Unset = chosen by batch size.
 * IYK_HIP_LATENCY_KERNEL = 0 / 3 is the older spelling of w32 / lat3.  IYK_HIP_KS_KERNEL = 0 / 1 / 2, read at every batch, forces
 * the key switch with 16 gates per workgroup (3 words per thread), the one with 16 gates per wave (whole rows per
 * wave, digits decoded by compare and branch; the default for batches of up to 4 096 gates, in its shared-gates form) or —
 * 2, the default for wider batches since round 6 — the one that takes the digits in pairs and selects a PRE-ADDED row by
 * address (a table of 16 sums per digit pair, built on the GPU from the resident key-switching key by the first wide batch:
 * + 136 MB per GPU, counted by iyk_hip_resident_key_bytes from then on); all three subtract the same rows mod 2^32, so
 * they agree word for word.  IYK_HIP_KS_KERNEL = 3 forces, at any batch size, the key switch as an integer matrix product on the
 * matrix cores (one-hot digits x the key's rows in four signed base-256 planes, v_mfma_i32_32x32x32_i8: nothing is rounded, the
 * words are the same again; no initialisation launch, no atomics).  Unset, batches of KS_MATRIX_MIN_JOBS (csrc/dispatch.hpp:
 * 4 608) gates or more run it, batches of 4 097 gates up to there the table of 2, narrower ones the shared-gates form of 1.
 * Its operand (73.4 MB per GPU at the 128-bit set, 67.1 MB at the 80-bit set) is built from the resident key by the first such
 * batch, on that batch's stream with stream-ordered allocation — no call blocks, the null stream is not touched — and counted by
 * iyk_hip_resident_key_bytes from then on.  IYK_HIP_KS_MATRIX_MAX_BYTES (read when the operand is first asked for) caps it: below
 * the operand's size, or when the allocation fails, the GPU remembers that it has no operand until the next iyk_hip_init and
 * every batch runs the form 0 / 1 / 2 would have chosen; no batch fails for it. */
int iyk_hip_ntt_path(void);

/* Round 4: return value 2 = the default since — both rotation kernels (a wave per rotation for full rounds, a workgroup per
 * rotation for narrow frontiers) multiply through a 512-point COMPLEX FP64 FFT with every key word split into two signed
 * 16-bit halves (csrc/fft512.hpp): every inverse-transform output is provably within 2^-8.5 (128-bit set) / 2^-5.1 (80-bit
 * set) of the exact integer sum for ANY key and digits, so rint() makes the product the exact schoolbook
 * one — the same ciphertext words as paths 1 and 0 — at two thirds of the instructions per CMUX step.  The field form of the
 * key is NOT resident on this path (round 6): the first batch that forces a field kernel (IYK_HIP_ROT_KERNEL = w32 / lat3, a
 * cross-check) builds it on that GPU from a host copy of the torus-domain key — one upload and one transform pass, synchronous —
 * and iyk_hip_resident_key_bytes grows by it from then on.  IYK_HIP_NTT = fft / fp / goldilocks at iyk_hip_init selects 2 / 1 / 0; IYK_HIP_ROT_KERNEL = fft / latfft
 * forces a batch onto one of the FFT kernels.  With IYK_HIP_DEBUG=1 at init the FFT kernels also record the largest
 * |z - rint(z)| they produced: */
int iyk_hip_fft_round_error(int gpu_index, double* out);

/* Digit polynomials per accumulator polynomial and CMUX step.  l on the integer path and for the 128-bit set; 2 l = 4 for
 * the 80-bit set on the FP64 path, whose 10-bit digits are split into 5-bit halves so that every integer sum stays below
 * p/2 UNCONDITIONALLY (the default).  IYK_HIP_DECOMP=direct at iyk_hip_init (80-bit set only, opt-in) uses the digits as
 * they are: l = 2, half the transforms and half the key stream, and the same ciphertexts unless an integer sum of 4096
 * digit x key-word products reaches p/2 — for real (uniform) key rows an event of probability <= 7e-24 per sum, 2e-17 per
 * gate whatever the digits (csrc/blind_rotate_fp.hpp has the bound), far below the scheme's own decryption-failure rate,
 * but not zero: a measured option, not the default.  There is no upstream counterpart (cuFHE's FFT is approximate anyway). */
int iyk_hip_decomposition_levels(void);

/* Identity of the build: 16 hex digits of the SHA-256 over the sources the library was compiled from (tools/src_hash.py;
 * "unknown" when built without -DIYK_BUILD_ID).  Measurement tooling stamps counter files with it, so that an
 * instruction count is never paired with a duration of a different kernel build. */
const char* iyk_hip_build_id(void);

/* Rotations one full round of the wave-per-rotation kernel holds on GPU `gpu_index` (8 resident waves per CU).  A scheduler
 * that can choose its batch sizes does best with multiples of it; the remainder of a batch goes to the workgroup-per-rotation
 * kernel (up to iyk_level_cost.max_passes passes) or one more partial round.
 * < 0 on error.  (cuFHE has no counterpart: it launches one gate per stream, /root/reference/src/iyokan_cufhe.hpp:249-258.) */
int iyk_hip_rotation_round(int gpu_index);

/* What a level of `rotations` blind rotations costs one GPU, as iyk_hip_gate_batch dispatches it: full rounds on the
 * wave-per-rotation kernel, a remainder of up to max_passes * pass rotations in passes of the narrow-frontier kernel (one
 * rotation per CU and pass), a larger remainder as one more round.  A scheduler that may choose which gates go into which
 * batch (iyokan_amd/frontier.py: plan_levels; host/iyokan_hip.hpp: planFrontiers) prices its choices with THIS table — the
 * library owns the only copy of the figures (round 3 had three).  _defaults: compiled-in MI355X figures of this build, no GPU
 * or initialisation needed; _table / _ms: GPU `gpu_index` of the initialised library (its CU count; measured values once
 * iyk_hip_calibrate(gpu_index) has run — ~0.15 s, also moves the dispatch's narrow-frontier threshold to the measured
 * cross-over).  build_id ties a table to the kernels it describes.  No upstream counterpart (cuFHE launches gate by gate). */
typedef struct iyk_level_cost {
    int32_t round;        /* rotations per full round of the wave-per-rotation kernel: 8 waves x CUs */
    int32_t pass;         /* rotations per pass of the narrow-frontier kernel: one per CU */
    int32_t max_passes;   /* remainders of up to max_passes * pass rotations go to the narrow-frontier kernel */
    int32_t calibrated;   /* 0: compiled-in figures, 1: measured on this GPU by iyk_hip_calibrate */
    float round_ms;       /* one round */
    float pass_ms[8];     /* pass_ms[j]: (j + 1) passes */
    char build_id[20];
} iyk_level_cost;
int iyk_hip_level_cost_defaults(iyk_level_cost* out);
int iyk_hip_level_cost_table(int gpu_index, iyk_level_cost* out);
double iyk_hip_level_cost_ms(int gpu_index, int rotations);
int iyk_hip_calibrate(int gpu_index);   /* gpu_index = -1: every GPU, concurrently (one host thread each) */

/* The steps of the last iyk_hip_init, "name [gpu] milliseconds" separated by ';': alloc g, pin, enqueue g, wait g.  Since round 5
 * the devices are fed CONCURRENTLY — buffers everywhere, the caller's key arrays page-locked once, uploads + key transforms
 * enqueued on one stream per device, then one wait per device — so every "enqueue" precedes the first "wait" and N GPUs cost about
 * what one costs (the reference replicates by a per-device loop inside cufhe::Initialize, /root/reference/src/iyokan_cufhe.cpp:530-536).
 * Valid until the next iyk_hip_init. */
const char* iyk_hip_init_profile(void);

/* Bytes of device memory holding keys on one GPU: the key spectra (FFT path) or the NTT-domain BK (field / integer paths), the
 * padded KSK and the tables — 179.8 MB at the 128-bit set on the default path — plus, once a cross-check kernel has asked for
 * it, the field form of the BK (62.5 MB; round 5 built and kept it at init: 242.3 MB) and, once a batch wider than 4 096 gates has
 * run on the table kernel, the key switch's table of pre-added rows (136 MB) and, once a batch has run the matrix form, its int8
 * operand (73.4 MB; both: IYK_HIP_KS_KERNEL above). */
int iyk_hip_resident_key_bytes(uint64_t* out);

/* The two FORMS of the lvl2 bootstrapping key object (iyk_hip_bk2_key_create above creates form 0).  The form is a property of the
 * key, because the device layouts differ; nothing is chosen per batch, and every output word is the same under either form.
 *   form 0  the integer key: the two 32-bit halves' spectra in Z_P (512 KiB per step); iyk_hip_cb_rotate_batch runs cb_rotate_kernel
 *           or cb_rotate_lat_kernel on it, as IYK_HIP_CB_KERNEL / dispatch::cb_plan say
 *   form 1  the FP64 key: the spectra of the four signed 16-bit quarters of every word, 1024 complex points each with the 1/1024 of
 *           the inverse transform folded in (1 MiB per step, 666 MB at n = 636); iyk_hip_cb_rotate_batch and
 *           iyk_hip_circuit_bootstrap_batch run cb_rotate_fft_kernel on it — exact by the proven rounding margin of DESIGN.md §2b (lvl2
 *           row).  IYK_HIP_CB_KERNEL = wg / lat changes nothing for such a key; any other value is still IYK_ERR_INVALID before
 *           anything is staged.  With IYK_HIP_DEBUG=1 the kernel feeds iyk_hip_fft_round_error.
 * Any other form, (l2, Bgbit2) != (4, 9), or form 1 on a device that did not grant the kernel its 160 KiB of LDS at iyk_hip_init, is
 * IYK_ERR_INVALID with a text that says which.  _upload, _free and _bytes serve both forms (the same host windows; _bytes counts both). */
int iyk_hip_bk2_key_create_form(int gpu_index, uint32_t n, uint32_t l2, uint32_t Bgbit2, int form, void** out);
int iyk_hip_bk2_key_form(const void* key, int* form_out);

/* Order one stream behind another on the device: everything enqueued on `st` after this call starts only once everything enqueued on
 * `other` BEFORE this call has finished.  An event is recorded on `other` and `st` waits for it; the host never blocks, and `other` is
 * not held up.  The event is one of a few `st` owns from its creation to iyk_hip_stream_destroy, used round-robin — a wait keeps the
 * record it was enqueued behind, so any number of waits may follow each other and nothing is created per call.  (A gate of
 * iyk_hip_gate_host that is still parked in a coalesced batch is not yet enqueued on `other` and is not waited for.)
 * What it is for: work that the next launches of one stream do not read — cmux.Ram's refresh of every cell — goes to a second stream
 * and is ordered back in front of its first reader ("refresh aside").
 * IYK_ERR_INVALID, with nothing enqueued on either stream and the reason in iyk_hip_last_error: a null stream, st == other, streams
 * on different GPUs, streams of different replicas of one GPU (a replica's stores and keys are its own).  The check is
 * args::stream_wait_args of csrc/batch_args.hpp.  No upstream counterpart: cuFHE's streams meet only on the host. */
int iyk_hip_stream_wait_stream(iyk_hip_stream* st, iyk_hip_stream* other);

#ifdef __cplusplus
}
#endif
#endif
