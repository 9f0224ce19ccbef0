#include "aecm_engine.h"

#include "aecm_host_rows.h"
#include "aecm_session_flow.h"
#include "aecm_state_check.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <thread>
#include <utility>
#include <vector>

namespace aecm {

#define AECM_HIP_OK(expr) ((expr) == hipSuccess)

bool GrowDeviceBuffer(void **buf, size_t *have, size_t need, size_t unit, hipStream_t stream) {
    if (need <= *have) return true;
    if (*buf && !AECM_HIP_OK(hipStreamSynchronize(stream))) return false;      // (nothing enqueued may still use the old one)
    (void)hipFree(*buf);
    *buf = nullptr;
    *have = 0;
    if (!AECM_HIP_OK(hipMalloc(buf, need * unit))) { *buf = nullptr; return false; }
    *have = need;
    return true;
}

// (kDefaultQueueChunk: launches of more streams than the chip holds waves are cut into chunks of that many blocks and scheduled from
// a queue -- aecm_block_kernels.hip: aecm_process_queue_kernel; measured: profiles/r04_experiments.md section 1.)

#if defined(AECM_EXPERIMENTS)
// Experiments build only (tools/ab_build.py adds -DAECM_EXPERIMENTS): the environment's wishes on top of the default policy, so that
// tools/sweep_streams.py and the A/B scripts can try launch forms without a caller that sets a policy.  The shipped library reads no
// environment variable anywhere.
static void ApplyEnvironmentWishes(LaunchPolicy *p) {
    auto num = [](const char *name, int *dst) { if (const char *env = getenv(name)) *dst = atoi(env); };
    if (const char *env = getenv("AECM_QUEUE_CHUNK")) p->queue_chunk_blocks = std::min(std::max(0, atoi(env)), BatchEngine::kMaxQueueChunk);
    num("AECM_QUEUE_MIN_STREAMS", &p->queue_min_streams);
    num("AECM_PIPE_FRONT", &p->pipe.front_waves);
    num("AECM_PIPE_TAIL", &p->pipe.tail_waves);
    num("AECM_PIPE_RAW", &p->pipe.raw);
    num("AECM_PIPE_DELAY", &p->pipe.delay_waves);
    num("AECM_PIPE_GAIN", &p->pipe.gain_waves);
    num("AECM_PIPE_SPREAD", &p->pipe.spread);
    num("AECM_PIPE_WGS", &p->pipe.wgs_per_cu);
    num("AECM_PIPE_ROT", &p->pipe.rot);
    num("AECM_PIPE_PRIO", &p->pipe.prio);
    num("AECM_PIPE_MAX_STREAMS", &p->pipelined_max_streams);
    if (const char *env = getenv("AECM_PIPELINED")) p->pipelined_min_streams = atoi(env) > 0 ? atoi(env) : 0x7fffffff;   // 0: off; n: from n streams
    if (const char *env = getenv("AECM_PIPE_MIN_BLOCKS")) p->pipelined_min_blocks = atoi(env) > 1 ? atoi(env) : 1;
}
#endif

// The launch-form limits of a device with `compute_units` CUs: everything follows from the CU count and from what the kernels are
// built for (waves per SIMD, LDS per workgroup: aecm_block_kernels.hip; tests/test_capi.py checks those against the code object).
LaunchPolicy DefaultLaunchPolicy(int compute_units) {
    LaunchPolicy p;
    p.compute_units = compute_units;
    p.rotation_stream_limit = RotationStreamLimit(compute_units);
    p.resident_waves = ResidentWaves(compute_units);
    p.pipelined_max_streams = PipelinedStreamLimit(compute_units, 0);      // the six-wave shape, four workgroups per CU
#if defined(AECM_EXPERIMENTS)
    ApplyEnvironmentWishes(&p);
#endif
    return p;
}

bool LaunchPolicyValid(const LaunchPolicy &p) {
    const PipeWishes &w = p.pipe;
    auto in = [](int v, std::initializer_list<int> ok) { return std::find(ok.begin(), ok.end(), v) != ok.end(); };
    return p.compute_units >= 0 && p.queue_chunk_blocks >= 0 && p.queue_chunk_blocks <= BatchEngine::kMaxQueueChunk && p.pipelined_min_blocks >= 1 &&
           p.pipelined_max_streams >= 0 && p.pipelined_max_streams <= PipelinedStreamLimit(p.compute_units, 0) && p.resident_waves > 0 &&
           p.resident_waves <= ResidentWaves(p.compute_units) && p.rotation_stream_limit >= 0 && in(w.tail_waves, {-1, 0, 2}) &&
           in(w.front_waves, {-1, 2, 4}) && in(w.raw, {-1, 0, 1}) && in(w.delay_waves, {-1, 0, 2, 4}) && in(w.gain_waves, {-1, 0, 4}) &&
           in(w.spread, {0, 1}) && w.wgs_per_cu >= 0 && w.wgs_per_cu <= 8 && w.rot >= -1 && w.rot < 1024 && w.prio >= -1 && w.prio < 256;
}

BatchEngine *BatchEngine::Create(int num_streams, int device_id) {
    if (num_streams <= 0) return nullptr;
    int n_dev = 0;
    if (!AECM_HIP_OK(hipGetDeviceCount(&n_dev)) || device_id < 0 || device_id >= n_dev) return nullptr;
    if (!AECM_HIP_OK(hipSetDevice(device_id))) return nullptr;
    BatchEngine *e = new BatchEngine();
    e->device_ = device_id;
    e->num_streams_ = num_streams;
    int cus = 0;
    if (!AECM_HIP_OK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device_id))) cus = 0;
    e->policy_ = DefaultLaunchPolicy(cus);
    const size_t S = (size_t)num_streams;
    bool ok = AECM_HIP_OK(hipStreamCreateWithFlags(&e->stream_, hipStreamNonBlocking)) &&
              AECM_HIP_OK(hipMalloc((void **)&e->st_.vec, S * kVecWordsPerStream * sizeof(uint32_t))) &&
              AECM_HIP_OK(hipMalloc((void **)&e->st_.scal, S * kNumScal * sizeof(int32_t))) &&
              AECM_HIP_OK(hipMalloc((void **)&e->st_.hist, S * kHistWordsPerStream * sizeof(uint16_t))) &&
              AECM_HIP_OK(hipMalloc((void **)&e->image_vec_dev_, kVecWordsPerStream * sizeof(uint32_t))) &&
              AECM_HIP_OK(hipMalloc((void **)&e->image_scal_dev_, kNumScal * sizeof(int32_t))) &&
              AECM_HIP_OK(hipMalloc((void **)&e->other_vec_dev_, kVecWordsPerStream * sizeof(uint32_t))) &&
              AECM_HIP_OK(hipMalloc((void **)&e->other_scal_dev_, kNumScal * sizeof(int32_t))) &&
              AECM_HIP_OK(hipMalloc((void **)&e->consts_dev_, kConstBlobWords * sizeof(uint32_t))) &&
              true;                                   // the timing events are created on first use (ProcessBlocks)
    if (ok) {
        // the 20 KB constants blob is built once per process (every WebRtcAecm_Create makes an engine of its own)
        static const std::vector<uint32_t> blob = [] { std::vector<uint32_t> b; BuildKernelConstants(&b); return b; }();
        ok = AECM_HIP_OK(hipMemcpy(e->consts_dev_, blob.data(), blob.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
        e->st_.consts = e->consts_dev_;
    }
    if (!ok) {
        delete e;
        return nullptr;
    }
    return e;
}

bool BatchEngine::set_launch_policy(const LaunchPolicy &p) {
    if (!LaunchPolicyValid(p) || p.compute_units != policy_.compute_units) return false;
    policy_ = p;
    return true;
}

BatchEngine::~BatchEngine() {
    (void)hipSetDevice(device_);
    if (stream_) (void)hipStreamSynchronize(stream_);
    for (int i = 0; i < kTimerSlots; ++i) {
        if (ev_start_[i]) (void)hipEventDestroy(ev_start_[i]);
        if (ev_stop_[i]) (void)hipEventDestroy(ev_stop_[i]);
    }
    (void)hipFree(st_.vec);
    (void)hipFree(st_.scal);
    (void)hipFree(st_.hist);
    (void)hipFree(image_vec_dev_);
    (void)hipFree(image_scal_dev_);
    (void)hipFree(other_vec_dev_);
    (void)hipFree(other_scal_dev_);
    (void)hipFree(select_dev_);
    (void)hipFree(consts_dev_);
    (void)hipFree(queue_ctl_);
    (void)hipFree(queue_err_);
    if (plan_host_) (void)hipHostFree(plan_host_);
    if (plan_uploaded_) (void)hipEventDestroy(plan_uploaded_);
    (void)hipFree(stage_dev_);
    if (mapped_host_) (void)hipHostFree(mapped_host_);
    (void)hipFree(rec_maps_);
    (void)hipFree(rec_scratch_);
    (void)hipFree(state_stage_);
    (void)hipFree(state_verdict_);
    if (download_stream_) (void)hipStreamDestroy(download_stream_);
    if (stream_) (void)hipStreamDestroy(stream_);
}

bool BatchEngine::Init(int fs) {
    StreamImage img, other;
    if (!BuildInitImage(fs, &img) || !BuildInitImage(fs == 8000 ? 16000 : 8000, &other)) return false;
    if (!AECM_HIP_OK(hipSetDevice(device_))) return false;
    if (!AECM_HIP_OK(hipMemcpyAsync(other_vec_dev_, other.vec.data(), other.vec.size() * sizeof(uint32_t), hipMemcpyHostToDevice, stream_)) ||
        !AECM_HIP_OK(hipMemcpyAsync(other_scal_dev_, other.scal.data(), other.scal.size() * sizeof(int32_t), hipMemcpyHostToDevice, stream_)))
        return false;
    if (!AECM_HIP_OK(hipMemcpyAsync(image_vec_dev_, img.vec.data(), img.vec.size() * sizeof(uint32_t),
                                    hipMemcpyHostToDevice, stream_)))
        return false;
    if (!AECM_HIP_OK(hipMemcpyAsync(image_scal_dev_, img.scal.data(), img.scal.size() * sizeof(int32_t),
                                    hipMemcpyHostToDevice, stream_)))
        return false;
    if (!AECM_HIP_OK(LaunchBroadcastImage(st_, image_vec_dev_, image_scal_dev_, 0, num_streams_, stream_))) return false;
    // a launch that failed (a wave of a chunk-queue launch gave up waiting: CheckQueueError) left the streams it had not
    // finished in an unknown state; re-initialising all of them is what clears the record
    if (queue_err_ && !AECM_HIP_OK(hipMemsetAsync(queue_err_, 0, sizeof(uint32_t), stream_))) return false;
    queue_unchecked_ = false;
    launch_failed_ = false;
    if (!AECM_HIP_OK(hipStreamSynchronize(stream_))) return false;   // img and other go out of scope
    initialized_ = true;
    fs_ = fs;
    mixed_rates_ = false;
    return true;
}

bool BatchEngine::InitStreams(int first, int count) {
    if (!initialized_ || first < 0 || count < 0 || first + count > num_streams_) return false;
    if (!AECM_HIP_OK(hipSetDevice(device_))) return false;
    // image_*_dev_ still hold the initial image of the last Init
    return AECM_HIP_OK(LaunchBroadcastImage(st_, image_vec_dev_, image_scal_dev_, first, count, stream_));
}

bool BatchEngine::InitStreamsAtRate(int first, int count, int fs) {
    if (fs == fs_) return InitStreams(first, count);
    if (!initialized_ || (fs != 8000 && fs != 16000) || first < 0 || count < 0 || first + count > num_streams_) return false;
    if (!AECM_HIP_OK(hipSetDevice(device_))) return false;
    if (count > 0) mixed_rates_ = true;
    return AECM_HIP_OK(LaunchBroadcastImage(st_, other_vec_dev_, other_scal_dev_, first, count, stream_));
}

bool BatchEngine::InitStreamsOfOtherRate(const int32_t *rates_host) {
    if (!initialized_) return false;
    std::vector<uint8_t> select((size_t)num_streams_);
    bool any = false;
    for (int s = 0; s < num_streams_; ++s) any |= (select[(size_t)s] = rates_host[s] != fs_) != 0;
    if (!any) return true;
    if (!AECM_HIP_OK(hipSetDevice(device_))) return false;
    if (!select_dev_ && !AECM_HIP_OK(hipMalloc((void **)&select_dev_, (size_t)num_streams_))) { select_dev_ = nullptr; return false; }
    mixed_rates_ = true;
    return AECM_HIP_OK(hipMemcpyAsync(select_dev_, select.data(), select.size(), hipMemcpyHostToDevice, stream_)) &&
           AECM_HIP_OK(LaunchBroadcastImageSelect(st_, other_vec_dev_, other_scal_dev_, select_dev_, num_streams_, stream_)) &&
           AECM_HIP_OK(hipStreamSynchronize(stream_));      // select goes out of scope
}

// Stream-ordered, no synchronisation: the next launch on the engine's stream sees the new values.
bool BatchEngine::PatchScalars(const int32_t *fields, const int32_t *values, int n, int first, int count) {
    if (n > kMaxPatchFields) return false;
    if (count < 0) count = num_streams_ - first;
    if (first < 0 || count < 0 || first + count > num_streams_) return false;
    if (!AECM_HIP_OK(hipSetDevice(device_))) return false;
    ScalarPatch patch{};
    patch.n = n;
    memcpy(patch.field, fields, n * sizeof(int32_t));
    memcpy(patch.value, values, n * sizeof(int32_t));
    return AECM_HIP_OK(LaunchPatchScalars(st_, patch, first, count, stream_));
}

bool BatchEngine::SetConfig(int cng_mode, int echo_mode, int first, int count) {
    int32_t scal[kNumScal] = {0};
    if (!ApplyConfig(scal, cng_mode, echo_mode)) return false;
    const int32_t fields[7] = {S_CNG, S_SUPGAIN, S_SUPGAIN_OLD, S_SG_A, S_SG_D, S_SG_DAB, S_SG_DBD};
    int32_t values[7];
    for (int i = 0; i < 7; ++i) values[i] = scal[fields[i]];
    return PatchScalars(fields, values, 7, first, count);
}

bool BatchEngine::SetCngMode(int cng_mode, int first, int count) {
    const int32_t fields[1] = {S_CNG};
    const int32_t values[1] = {cng_mode};
    return PatchScalars(fields, values, 1, first, count);
}

bool BatchEngine::Control(int fixed_delay, int nlp_flag, int first, int count) {
    int32_t scal[kNumScal] = {0};
    ApplyControl(scal, fixed_delay, nlp_flag);
    const int32_t fields[2] = {S_NLP, S_FIXED_DELAY};
    const int32_t values[2] = {scal[S_NLP], scal[S_FIXED_DELAY]};
    return PatchScalars(fields, values, 2, first, count);
}

// Collect the durations of finished launches.  wait_all: block until every pending pair has completed
// (getters); otherwise take only what has already finished -- never blocks.
bool BatchEngine::HarvestTimers(bool wait_all) {
    while (timer_pending_ > 0) {
        const int slot = timer_head_;
        if (wait_all) {
            if (!AECM_HIP_OK(hipEventSynchronize(ev_stop_[slot]))) return false;
        } else {
            const hipError_t q = hipEventQuery(ev_stop_[slot]);
            if (q == hipErrorNotReady) return true;
            if (q != hipSuccess) return false;
        }
        float ms = 0.f;
        if (!AECM_HIP_OK(hipEventElapsedTime(&ms, ev_start_[slot], ev_stop_[slot]))) return false;
        last_ms_ = ms;
        total_ms_ += ms;
        launches_ += 1;
        timer_head_ = (timer_head_ + 1) % kTimerSlots;
        --timer_pending_;
    }
    return true;
}

// The word a wave of a chunk-queue or pipelined launch raises when it gives up waiting for another wave (never cleared by a launch).
bool BatchEngine::EnsureLaunchErrorWord() {
    if (queue_err_) return true;
    return AECM_HIP_OK(hipMalloc((void **)&queue_err_, sizeof(uint32_t))) && AECM_HIP_OK(hipMemsetAsync(queue_err_, 0, sizeof(uint32_t), stream_));
}

// The control words of a chunk-queue or pipelined launch (one buffer, grown on first use; launches on stream_ are ordered, so
// consecutive launches may share it).
bool BatchEngine::EnsureLaunchControl(size_t need) {
    if (need <= queue_ctl_bytes_) return true;
    if (!AECM_HIP_OK(hipStreamSynchronize(stream_))) return false;       // stream-ordered work may still read the old one
    (void)hipFree(queue_ctl_);
    queue_ctl_ = nullptr;
    queue_ctl_bytes_ = 0;
    if (!AECM_HIP_OK(hipMalloc((void **)&queue_ctl_, need))) return false;
    queue_ctl_bytes_ = need;
    return true;
}

// Which form a launch of `count` streams x num_blocks blocks takes under a policy (host logic, no device): the rules of
// INTEGRATION.md's table, held by PlanLaunch and PlanRaggedLaunch and by nothing else.
//   chunk queue   every launch of more streams than the pipelined form takes (or than queue_min_streams, when set) that is at least
//                 two chunks long: above the chip's resident waves because the launch would otherwise end in a long drain, and between
//                 4 096 streams and that too -- every wave is resident there, but the SIMD's arbiter favours its oldest wave, the waves
//                 dispatched first pull ahead, and with items claimed in order those waves simply take more of the work (4 608 streams
//                 728 -> 830 M frames/s, 6 144: 844 -> 930 M; profiles/r04_experiments.md section 4).  Shorter chunks there: a quarter.
//   pipelined     launches the chip holds at once: fast variant, every stream the same number of blocks, and no clean input unless the
//                 batch has opted in (set_clean_pipelining: aecm_process_pipelined_clean_kernel); ragged launches by the live streams
//                 and the longest length, on a batch that has opted in (set_ragged_pipelining without a clean input,
//                 set_ragged_clean_pipelining with one: aecm_process_pipelined_ragged_clean_kernel)
//   else          one wavefront per stream: by phase priority (form 1) when the launch is more waves than the rotation kernels are built for
namespace {
int QueueMinStreams(const LaunchPolicy &p) { return p.queue_min_streams >= 0 ? p.queue_min_streams : p.pipelined_max_streams; }
// (The quarter rule is for the default chunk; a length set by the caller is taken as it is.)
int QueueChunkFor(const LaunchPolicy &p, int count) {
    if (p.queue_chunk_blocks <= 0 || count > p.resident_waves || p.queue_chunk_explicit) return p.queue_chunk_blocks;
    return std::max(8, p.queue_chunk_blocks / 4);
}
bool PipelinedLaunchApplies(const LaunchPolicy &p, int variant, int count, int num_blocks, bool clean, bool clean_pipelining) {
    return variant == kVariantFast && (!clean || clean_pipelining) && count >= p.pipelined_min_streams && count <= p.pipelined_max_streams &&
           num_blocks >= p.pipelined_min_blocks;
}
int WavePerStreamForm(const LaunchPolicy &p, int variant, int count) { return variant == kVariantFast && count > p.rotation_stream_limit ? 1 : 0; }
int PipeShapeBits(const PipeShape &sh) {
    return sh.tail_waves | (sh.balance ? 0x100 : 0) | (sh.front_waves == 4 ? 0x200 : 0) | (sh.raw ? 0x400 : 0) | (sh.delay_waves ? 0x800 : 0) |
           (sh.gain_waves ? 0x1000 : 0);
}
constexpr int kPipeShapeCleanBit = 0x2000;        // the launch runs aecm_process_pipelined_clean_kernel (ragged: _ragged_clean_kernel)
int RoundsX1000(int workgroups, int cus, int workgroups_per_cu) { return (int)((int64_t)1000 * workgroups / ((int64_t)cus * std::max(1, workgroups_per_cu))); }
// The control buffer a ragged plan needs: the pipelined form's plan alone, else the queue's control words with the plan behind them.
size_t RaggedControlBytes(const LaunchPlan &plan) {
    return plan.form == 3 ? plan.pipe.words.size() * sizeof(uint32_t) : RaggedQueueControlBytes(plan.count, plan.ragged.n_chunks);
}
LaunchPlan UndecidedPlan(int variant, int count, int num_blocks, bool has_clean) {
    LaunchPlan plan;
    plan.variant = variant, plan.count = count, plan.num_blocks = num_blocks, plan.has_clean = has_clean;
    return plan;
}
}  // namespace

LaunchPlan PlanLaunch(const LaunchPolicy &p, const LaunchSwitches &sw, int count, int num_blocks, bool has_clean) {
    LaunchPlan plan = UndecidedPlan(sw.variant, count, num_blocks, has_clean);
    plan.trace = sw.trace;
    const int chunk = QueueChunkFor(p, count);
    if (QueueLaunchApplies(count, num_blocks, sw.variant, chunk, QueueMinStreams(p))) {
        plan.form = 2;
        plan.chunk_blocks = chunk;
    } else if (!sw.trace && PipelinedLaunchApplies(p, sw.variant, count, num_blocks, has_clean, sw.clean_pipelining)) {      // (no traced pipelined form)
        plan.form = 3;
        plan.shape = has_clean ? PipelinedCleanShapeFor(count, num_blocks, p.compute_units, p.pipe) : PipelinedShapeFor(count, num_blocks, p.compute_units, p.pipe);
    } else {
        plan.form = WavePerStreamForm(p, sw.variant, count);
    }
    return plan;
}

LaunchDescription DescribePlan(const LaunchPolicy &p, const LaunchPlan &plan) {
    LaunchDescription d;
    d.form = plan.form < 0 ? -1 : plan.form;
    if (plan.form < 0 || (plan.is_ragged && plan.num_blocks == 0)) return d;      // refused lengths; nothing to launch
    const int cus = p.compute_units > 0 ? p.compute_units : 256;
    if (plan.form == 2) {
        d.chunk_blocks = plan.chunk_blocks;
        d.waves_per_workgroup = kWavesPerWorkgroup;
        d.workgroups = QueueGridWorkgroups(plan.is_ragged ? plan.ragged.live_streams : plan.count, p.resident_waves);
        d.workgroups_per_cu = std::max(p.resident_waves / (cus * kWavesPerWorkgroup), 1);
    } else if (plan.form == 3) {
        const PipeShape &sh = plan.shape;
        d.shape = PipeShapeBits(sh) | (plan.has_clean ? kPipeShapeCleanBit : 0);
        d.workgroups = plan.is_ragged ? plan.pipe.workgroups : sh.workgroups;
        d.waves_per_workgroup = PipelinedWorkgroupWaves(sh);
        d.workgroups_per_cu = p.pipe.wgs_per_cu > 0 ? p.pipe.wgs_per_cu : PipelinedWorkgroupsPerCu(sh);
        if (plan.is_ragged) {
            d.cu_load_evenness_x1000 = plan.pipe.evenness_x1000();
        } else {
            // workgroups i, i + CUs, ... share a CU (the dispatcher deals them out in turn); the first count % workgroups serve one stream more
            const int count = plan.count, base = count / sh.workgroups, rem = count % sh.workgroups;
            int fullest = 0;
            for (int c = 0; c < std::min(cus, sh.workgroups); ++c) {
                int load = 0;
                for (int w = c; w < sh.workgroups; w += cus) load += base + (w < rem ? 1 : 0);
                fullest = std::max(fullest, load);
            }
            d.cu_load_evenness_x1000 = (int)((int64_t)1000 * count / ((int64_t)std::max(fullest, 1) * std::min(cus, sh.workgroups)));
        }
    } else {
        d.waves_per_workgroup = kWavesPerWorkgroup;
        d.workgroups = (plan.count + kWavesPerWorkgroup - 1) / kWavesPerWorkgroup;
        d.workgroups_per_cu = (plan.form == 1 ? p.resident_waves : std::max(p.rotation_stream_limit, 1)) / (cus * kWavesPerWorkgroup);
    }
    d.rounds_x1000 = RoundsX1000(d.workgroups, cus, d.workgroups_per_cu);
    return d;
}

// The plan of a ragged launch (aecm_engine.h: RaggedPlan; read by aecm_process_ragged_queue_kernel).  A counting sort by length --
// O(S + num_blocks), stable, longest first -- so that a plan for 65 536 streams costs well under a millisecond of host time.
bool BuildRaggedPlan(const int32_t *lens, int S, int num_blocks, int chunk_blocks, RaggedPlan *plan) {
    RaggedPlan &p = *plan;
    p = RaggedPlan();
    if (S < 0 || num_blocks < 0) return false;
    p.num_streams = S;
    p.chunk_blocks = chunk_blocks > 0 ? chunk_blocks : 0;
    std::vector<uint32_t> at((size_t)num_blocks + 2, 0u);       // at[l]: streams longer than l, i.e. the rank of the first stream of length l
    for (int s = 0; s < S; ++s) {
        const int32_t l = lens[s];
        if (l < 0 || l > num_blocks) return false;
        at[l] += 1;
        p.sum_blocks += l;
        p.max_blocks = std::max(p.max_blocks, (int)l);
        if (l > 0) {
            p.live_streams += 1;
            if (p.chunk_blocks) p.items += (l + p.chunk_blocks - 1) / p.chunk_blocks;
        }
    }
    p.n_chunks = p.chunk_blocks ? (p.max_blocks + p.chunk_blocks - 1) / p.chunk_blocks : 0;
    const bool with_items = p.items < (int64_t(1) << 31);
    p.words.assign(2 * (size_t)S + (with_items ? (size_t)p.n_chunks + 1 : 1), 0u);
    uint32_t longer = 0;                                          // counts -> ranks: exclusive suffix sums
    for (int l = num_blocks; l >= 0; --l) {
        const uint32_t n = at[l];
        at[l] = longer;
        longer += n;
    }
    uint32_t *len = p.words.data(), *order = len + S, *first_item = order + S;
    if (with_items)                                               // live[c] = streams longer than c x chunk = the rank of the first stream of that length or less
        for (int c = 0; c < p.n_chunks; ++c) first_item[c + 1] = first_item[c] + at[(size_t)c * p.chunk_blocks];
    for (int s = 0; s < S; ++s) {
        len[s] = (uint32_t)lens[s];
        order[at[lens[s]]++] = (uint32_t)s;
    }
    return true;
}

PipeShape RaggedPipeShapeFor(int live, int max_blocks, int compute_units, const PipeWishes &wishes) {
    PipeShape sh = PipelinedShapeFor(live, max_blocks, compute_units, wishes);
    if (sh.balance) {                 // the size that picks the balanced six-wave shape takes the plain one (no ragged instantiation of it)
        sh.balance = false;
        sh.raw = false;
    }
    return sh;
}

// The plan of a ragged pipelined launch (aecm_engine.h: RaggedPipePlan).  O(S + longest) for the order (BuildRaggedPlan's counting
// sort), O(live x log cus) for the placement.
bool BuildRaggedPipePlan(const int32_t *lens, int S, const PipeShape &shape, int compute_units, RaggedPipePlan *plan) {
    RaggedPipePlan &p = *plan;
    p = RaggedPipePlan();
    p.shape = shape;
    if (S <= 0 || !lens || shape.balance || shape.workgroups <= 0) return false;
    int longest = 0;
    for (int s = 0; s < S; ++s) {
        if (lens[s] < 0) return false;
        longest = std::max(longest, (int)lens[s]);
    }
    RaggedPlan sorted;
    if (!BuildRaggedPlan(lens, S, longest, 0, &sorted) || sorted.live_streams == 0) return false;
    const int cus = compute_units > 0 ? compute_units : 256, W = shape.workgroups, live = sorted.live_streams;
    if ((int64_t)W * 4 < live) return false;
    p.num_streams = S;
    p.live_streams = live;
    p.max_blocks = sorted.max_blocks;
    p.sum_blocks = sorted.sum_blocks;
    p.used_cus = std::min(cus, W);
    // longest first onto the unit with the fewest blocks that has a free slot: a min-heap of (blocks, unit); a full unit leaves it
    std::vector<std::vector<uint32_t>> of_cu((size_t)p.used_cus);
    std::vector<std::pair<int64_t, int>> heap;
    heap.reserve((size_t)p.used_cus);
    for (int c = 0; c < p.used_cus; ++c) heap.emplace_back(0, c);
    auto later = [](const std::pair<int64_t, int> &a, const std::pair<int64_t, int> &b) { return a > b; };      // (heap of the smallest)
    const auto wgs_of = [&](int c) { return (W - c + cus - 1) / cus; };      // workgroups c, c + cus, ... < W
    const uint32_t *order = sorted.order();
    for (int r = 0; r < live; ++r) {
        const uint32_t s = order[r];
        std::pop_heap(heap.begin(), heap.end(), later);
        std::pair<int64_t, int> &least = heap.back();
        of_cu[(size_t)least.second].push_back(s);
        least.first += lens[s];
        p.fullest_cu_blocks = std::max(p.fullest_cu_blocks, least.first);
        if ((int)of_cu[(size_t)least.second].size() == 4 * wgs_of(least.second)) heap.pop_back();
        else std::push_heap(heap.begin(), heap.end(), later);
    }
    // a unit's streams (already longest first) in consecutive runs over its workgroups; slots 0, 2, 1, 3 by length
    static const int kSlotOrder[4] = {0, 2, 1, 3};
    std::vector<int32_t> slots((size_t)W * 4, -1);
    for (int c = 0; c < p.used_cus; ++c) {
        const std::vector<uint32_t> &mine = of_cu[(size_t)c];
        const int g = wgs_of(c), n = (int)mine.size(), base = n / g, rem = n % g;
        int at = 0;
        for (int j = 0; j < g; ++j) {
            const int wg = c + j * cus, take = base + (j < rem ? 1 : 0);
            for (int k = 0; k < take; ++k) slots[(size_t)wg * 4 + kSlotOrder[k]] = (int32_t)mine[(size_t)at + k];
            at += take;
            if (take > 0) p.workgroups = std::max(p.workgroups, wg + 1);
        }
    }
    p.words.resize((size_t)p.workgroups * 4 + (size_t)S);
    for (size_t i = 0; i < (size_t)p.workgroups * 4; ++i) p.words[i] = (uint32_t)slots[i];
    for (int s = 0; s < S; ++s) p.words[(size_t)p.workgroups * 4 + s] = (uint32_t)lens[s];
    return true;
}

LaunchPlan PlanRaggedLaunch(const LaunchPolicy &p, const LaunchSwitches &sw, int count, int num_blocks, const int32_t *lens, bool has_clean) {
    LaunchPlan plan;
    // one pass over the lengths decides the form; the ragged plan is then built once, with the chunk that form runs by
    int live = 0, longest = 0;
    int64_t sum = 0;
    bool valid = count >= 0 && num_blocks >= 0 && (lens || count == 0);
    for (int s = 0; valid && s < count; ++s) {
        valid = lens[s] >= 0 && lens[s] <= num_blocks;
        live += lens[s] > 0;
        longest = std::max(longest, (int)lens[s]);
        sum += lens[s];
    }
    if (!valid) { plan.form = -1; return plan; }
    if (longest > 0 && sum == (int64_t)count * longest) {         // every stream the same length: the equal-length launch, whatever its form
        plan = PlanLaunch(p, sw, count, longest, has_clean);       // (the ragged plan then tells the caller the queue's item count)
    } else {
        plan = UndecidedPlan(sw.variant, count, longest, has_clean);      // (longest 0: nothing to launch)
        plan.is_ragged = true;
        plan.trace = sw.trace;
        // the queue over the live streams; else -- the opt-in -- a launch the chip holds at once pipelined, by the LIVE streams, not the
        // batch's size; else one wavefront per stream of the whole range, each with its own count (a wave of a zero-length stream leaves at once)
        const int chunk = QueueChunkFor(p, live);
        if (QueueLaunchApplies(live, longest, sw.variant, chunk, QueueMinStreams(p))) {
            plan.form = 2;
            plan.chunk_blocks = chunk;
        } else if (longest > 0) {
            plan.form = WavePerStreamForm(p, sw.variant, count);
            // (a clean input: by a switch of its own, in the clean shapes -- the other two switches leave such a launch as it is)
            const bool opted_in = !sw.trace && (has_clean ? sw.ragged_clean_pipelining : sw.ragged_pipelining);      // (no traced pipelined form)
            if (opted_in && PipelinedLaunchApplies(p, sw.variant, live, longest, has_clean, has_clean)) {
                plan.shape = has_clean ? PipelinedCleanShapeFor(live, longest, p.compute_units, p.pipe) : RaggedPipeShapeFor(live, longest, p.compute_units, p.pipe);
                if (BuildRaggedPipePlan(lens, count, plan.shape, p.compute_units, &plan.pipe)) plan.form = 3;
            }
        }
    }
    BuildRaggedPlan(lens, count, num_blocks, plan.form == 2 ? plan.chunk_blocks : 0, &plan.ragged);
    return plan;
}

// A tick of a session batch (aecm_kernels.hip: aecm_tick_flow_kernel): one wavefront per session, four per workgroup, seven such
// workgroups per CU -- 65 536 sessions on 256 CUs are 16 384 workgroups on 1 792 places: 9.14 rounds, the last one 14 % full.
LaunchDescription DescribeTickLaunch(int num_sessions, int compute_units) {
    LaunchDescription d;
    const int cus = compute_units > 0 ? compute_units : 256;
    d.form = 0;
    d.waves_per_workgroup = TickWorkgroupWaves();
    d.workgroups = (num_sessions + d.waves_per_workgroup - 1) / d.waves_per_workgroup;
    d.workgroups_per_cu = TickWorkgroupsPerCu();
    d.rounds_x1000 = RoundsX1000(d.workgroups, cus, d.workgroups_per_cu);
    return d;
}
// The same for a tick in which only live_sessions of the object's sessions call (aecm_tick_flow_sparse_kernel): the grid, and
// with it the rounds, are by the sessions that call; none at all when nobody does.
LaunchDescription DescribeTickLaunchLive(int num_sessions, int live_sessions, int compute_units) {
    if (live_sessions >= num_sessions) return DescribeTickLaunch(num_sessions, compute_units);
    LaunchDescription d = DescribeTickLaunch(live_sessions > 0 ? live_sessions : 1, compute_units);
    if (live_sessions <= 0) {
        d.workgroups = 0;
        d.rounds_x1000 = 0;
    }
    return d;
}

// The plan travels through a pinned buffer of the engine's, so the copy is asynchronous and the caller's (and the plan's) memory is
// free when this returns; the buffer is reused once the previous upload has run.
// (Grown, and the event created, on first use -- by ProcessBlocksRaggedRange ahead of the launch's timing events, so that no
// allocation falls between them.  Growing waits for the previous upload: the old buffer may still be read.)
bool BatchEngine::EnsurePlanStaging(size_t words) {
    if (words > plan_host_words_) {
        if (plan_upload_pending_) {
            if (!AECM_HIP_OK(hipEventSynchronize(plan_uploaded_))) return false;
            plan_upload_pending_ = false;
        }
        if (plan_host_) (void)hipHostFree(plan_host_);
        plan_host_ = nullptr;
        plan_host_words_ = 0;
        if (!AECM_HIP_OK(hipHostMalloc((void **)&plan_host_, words * sizeof(uint32_t), hipHostMallocDefault))) return false;
        plan_host_words_ = words;
    }
    return plan_uploaded_ || AECM_HIP_OK(hipEventCreateWithFlags(&plan_uploaded_, hipEventDisableTiming));
}

bool BatchEngine::UploadPlanWords(const std::vector<uint32_t> &plan_words, uint32_t *dst_dev) {
    const size_t words = plan_words.size();
    if (plan_upload_pending_) {
        if (!AECM_HIP_OK(hipEventSynchronize(plan_uploaded_))) return false;
        plan_upload_pending_ = false;
    }
    if (!EnsurePlanStaging(words)) return false;
    memcpy(plan_host_, plan_words.data(), words * sizeof(uint32_t));
    if (!AECM_HIP_OK(hipMemcpyAsync(dst_dev, plan_host_, words * sizeof(uint32_t), hipMemcpyHostToDevice, stream_))) return false;
    if (!AECM_HIP_OK(hipEventRecord(plan_uploaded_, stream_))) return false;
    plan_upload_pending_ = true;
    return true;
}

// One launch of the block kernels: the plan's form on the plan's streams (st, io already offset to the first of them).
bool BatchEngine::LaunchBlocks(const StatePtrs &st, const IoView &io, const LaunchPlan &plan) {
    if (launch_failed_) return false;                 // streams half processed by an abandoned launch: nothing runs until Init
    if (plan.form < 0 || plan.has_clean != (io.near_clean != nullptr)) return false;      // not the plan of this launch
    if (plan.trace && (plan.form == 3 || !trace_.records)) return false;                  // (PlanLaunch never makes the first; the second: detached since)
    const int count = plan.count, num_blocks = plan.num_blocks;
    const int32_t *lens_dev = nullptr;
    if (plan.is_ragged) {
        // one upload per launch, on the engine's stream.  Pipelined: the plan (slots, then lengths) at the start of the control buffer; no
        // control words, nothing to clear.  Else behind the control words the queue form clears: the whole plan for the queue, for one
        // wavefront per stream its first part (the lengths) is what aecm_process_kernel reads
        if (plan.form == 3 && plan.pipe.num_streams != count) return false;
        if (!EnsureLaunchControl(RaggedControlBytes(plan))) return false;
        uint32_t *plan_dev = queue_ctl_ + (plan.form == 3 ? 0 : RaggedPlanOffsetWords(count));
        if (!UploadPlanWords(plan.words(), plan_dev)) return false;
        lens_dev = reinterpret_cast<const int32_t *>(plan_dev);
    }
    switch (plan.form) {
    case 2:
        if (!plan.is_ragged && !EnsureLaunchControl(QueueControlBytes(count))) return false;
        if (!EnsureLaunchErrorWord()) return false;
        queue_unchecked_ = true;
        if (plan.trace) {
            if (plan.is_ragged)
                return AECM_HIP_OK(LaunchTraceBlocksRaggedQueued(st, io, trace_, count, plan.ragged.live_streams, (uint32_t)plan.ragged.items, plan.chunk_blocks,
                                                                 policy_.resident_waves, queue_ctl_, queue_err_, stream_));
            return AECM_HIP_OK(LaunchTraceBlocksQueued(st, io, trace_, count, num_blocks, plan.chunk_blocks, policy_.resident_waves, queue_ctl_, queue_err_, stream_));
        }
        if (plan.is_ragged)
            return AECM_HIP_OK(LaunchProcessBlocksRaggedQueued(st, io, count, plan.ragged.live_streams, (uint32_t)plan.ragged.items, plan.chunk_blocks,
                                                               policy_.resident_waves, queue_ctl_, queue_err_, stream_));
        return AECM_HIP_OK(LaunchProcessBlocksQueued(st, io, count, num_blocks, plan.chunk_blocks, policy_.resident_waves, queue_ctl_, queue_err_, stream_));
    case 3: {
        if (plan.is_ragged) return AECM_HIP_OK(LaunchProcessBlocksPipelinedRagged(st, io, count, plan.shape, plan.pipe.workgroups, queue_ctl_, stream_));
        bool need_ctl = plan.shape.balance;
#if defined(AECM_PIPE_TRACE)
        need_ctl = true;                      // (the diagnostics build keeps the buffer: its per-wave records live behind the progress words)
        trace_streams_ = plan.shape.workgroups;
#endif
        if (need_ctl && !EnsureLaunchControl(PipelinedControlBytes(plan.shape.workgroups))) return false;
        return AECM_HIP_OK(LaunchProcessBlocksPipelined(st, io, count, num_blocks, plan.shape, need_ctl ? queue_ctl_ : nullptr, stream_));
    }
    default:
        if (plan.trace) return AECM_HIP_OK(LaunchTraceBlocks(st, io, trace_, count, num_blocks, plan.variant, plan.form == 1, stream_, lens_dev));
        return AECM_HIP_OK(LaunchProcessBlocks(st, io, count, num_blocks, plan.variant, plan.form == 1, stream_, lens_dev));
    }
}

int32_t BatchEngine::SetBlockTrace(void *trace_dev, int64_t stream_stride, int64_t block_stride) {
    if (!trace_dev) {
        trace_ = TraceView{nullptr, 0, 0};
        switches_.trace = false;
        return 0;
    }
    // the kernels store the records as 32-bit words: a pointer that is not a multiple of 4 would fault on the GPU
    if ((reinterpret_cast<uintptr_t>(trace_dev) & 3) || stream_stride <= 0 || block_stride <= 0) return kErrBadParameter;
    trace_ = TraceView{static_cast<uint32_t *>(trace_dev), stream_stride, block_stride};
    switches_.trace = true;
    return 0;
}

int BatchEngine::DescribeLaunch(int num_blocks, bool has_clean, int *chunk_blocks) const {
    const LaunchDescription d = DescribePlan(policy_, PlanLaunch(policy_, switches_, num_streams_, num_blocks, has_clean));
    if (chunk_blocks) *chunk_blocks = d.detail();
    return d.form;
}

// Wait for everything enqueued on stream_; false if a HIP call failed or a wave of a chunk-queue launch gave up waiting.
bool BatchEngine::Drain() {
    if (!AECM_HIP_OK(hipStreamSynchronize(stream_))) return false;
#if defined(AECM_PIPE_TRACE)     // diagnostics build: the last pipelined launch's per-wave records -> $AECM_PIPE_TRACE_FILE (raw uint64 x 4 per wave)
    if (const char *path = getenv("AECM_PIPE_TRACE_FILE")) {
        if (trace_streams_ > 0) {
            const size_t off = PipelinedTraceOffsetBytes(trace_streams_), bytes = PipelinedControlBytes(trace_streams_) - off;
            std::vector<uint8_t> host(bytes);
            if (AECM_HIP_OK(hipMemcpy(host.data(), reinterpret_cast<uint8_t *>(queue_ctl_) + off, bytes, hipMemcpyDeviceToHost))) {
                if (FILE *f = fopen(path, "wb")) { fwrite(host.data(), 1, bytes, f); fclose(f); }
            }
            trace_streams_ = 0;
        }
    }
#endif
    return CheckQueueError();
}

// After a synchronisation of stream_: did a wave of a chunk-queue launch give up waiting (it never should)?  The verdict
// is sticky: an abandoned launch leaves streams half processed, so every later Drain() (ExportState, Digest, GetEchoPath,
// Synchronize ...) and every later launch fails too, until Init() has re-initialised the streams.
bool BatchEngine::CheckQueueError() {
    if (launch_failed_) return false;
    if (!queue_unchecked_) return true;
    uint32_t err = 0;
    if (!AECM_HIP_OK(hipMemcpy(&err, queue_err_, sizeof err, hipMemcpyDeviceToHost))) return false;      // unchecked stays set: asked again next time
    queue_unchecked_ = false;
    if (err != 0) launch_failed_ = true;
    return err == 0;
}

bool BatchEngine::ProcessBlocks(const IoView &io, int num_blocks, const int32_t *retired) {
    return !retired && ProcessBlocksRange(io, num_blocks, 0, num_streams_);
}

// Streams [first, first + count); io is indexed from `first`.
bool BatchEngine::ProcessBlocksRange(const IoView &io, int num_blocks, int first, int count) {
    return TimedLaunch(io, first, PlanLaunch(policy_, switches_, count, num_blocks, io.near_clean != nullptr));
}

int32_t BatchEngine::ProcessBlocksRagged(const IoView &io, int num_blocks, const int32_t *blocks_per_stream_host) {
    return ProcessBlocksRaggedRange(io, num_blocks, 0, num_streams_, blocks_per_stream_host);
}

int32_t BatchEngine::ProcessBlocksRaggedRange(const IoView &io, int num_blocks, int first, int count, const int32_t *lens) {
    if (first < 0 || count < 0 || first + count > num_streams_ || num_blocks < 0 || !lens) return kErrBadParameter;
    const LaunchPlan plan = PlanRaggedLaunch(policy_, switches_, count, num_blocks, lens, io.near_clean != nullptr);
    if (plan.form < 0) return kErrBadParameter;
    if (plan.num_blocks == 0) return 0;
    // (allocations ahead of the launch's timing events)
    if (plan.is_ragged && (!AECM_HIP_OK(hipSetDevice(device_)) || !EnsureLaunchControl(RaggedControlBytes(plan)) || !EnsurePlanStaging(plan.words().size())))
        return kErrUnspecified;
    return TimedLaunch(io, first, plan) ? 0 : kErrUnspecified;
}

// Host audio: the live blocks are packed into dense device rows (zeros behind a stream's length), run, and the blocks that
// were written are copied back.
int32_t BatchEngine::ProcessBlocksRaggedHost(const IoView &io, int num_blocks, const int32_t *lens) {
    if (switches_.trace) return kErrUnsupported;      // the block trace is for device-pointer launches
    if (num_blocks < 0 || !lens) return kErrBadParameter;
    for (int s = 0; s < num_streams_; ++s)
        if (lens[s] < 0 || lens[s] > num_blocks) return kErrBadParameter;
    if (num_blocks == 0) return 0;
    if (!AECM_HIP_OK(hipSetDevice(device_))) return kErrUnspecified;
    const RowLayout rows{num_streams_, num_blocks, io.stream_stride, io.block_stride};
    const size_t per = rows.per(), bytes = per * sizeof(int16_t);
    const bool has_clean = io.near_clean != nullptr;
    if (!GrowDeviceBuffer((void **)&stage_dev_, &stage_elems_, StagedSamples(per, has_clean), sizeof(int16_t), stream_)) return kErrUnspecified;
    const IoView dev = StagedIo(stage_dev_, rows.row(), per, has_clean);
    std::vector<int16_t> tmp(per, 0);
    auto upload = [&](const int16_t *src, const int16_t *dst) -> bool {
        PackRows(rows, src, tmp.data(), lens);
        return AECM_HIP_OK(hipMemcpy(const_cast<int16_t *>(dst), tmp.data(), bytes, hipMemcpyHostToDevice));
    };
    if (!upload(io.far, dev.far) || !upload(io.near, dev.near) || (has_clean && !upload(io.near_clean, dev.near_clean))) return kErrUnspecified;
    if (const int32_t rc = ProcessBlocksRagged(dev, num_blocks, lens)) return rc;
    if (!AECM_HIP_OK(hipMemcpyAsync(tmp.data(), dev.out, bytes, hipMemcpyDeviceToHost, stream_))) {
        (void)Drain();                                                // tmp goes out of scope
        return kErrUnspecified;
    }
    if (!Drain()) return kErrUnspecified;
    UnpackRows(rows, tmp.data(), io.out, lens);
    return 0;
}

bool BatchEngine::TimedLaunch(const IoView &io, int first, const LaunchPlan &plan) {
    if (first < 0 || plan.count < 0 || first + plan.count > num_streams_) return false;
    if (!AECM_HIP_OK(hipSetDevice(device_))) return false;
    if (!HarvestTimers(false)) return false;
    if (timer_pending_ == kTimerSlots) {         // ring full: wait for the oldest launch only
        if (!AECM_HIP_OK(hipEventSynchronize(ev_stop_[timer_head_])) || !HarvestTimers(false)) return false;
    }
    const int slot = (timer_head_ + timer_pending_) % kTimerSlots;
    if (!ev_start_[slot] && (!AECM_HIP_OK(hipEventCreate(&ev_start_[slot])) || !AECM_HIP_OK(hipEventCreate(&ev_stop_[slot])))) return false;
    if (!AECM_HIP_OK(hipEventRecord(ev_start_[slot], stream_))) return false;
    StatePtrs st = st_;
    st.vec += (size_t)first * kVecWordsPerStream;
    st.scal += (size_t)first * kNumScal;
    st.hist += (size_t)first * kHistWordsPerStream;
    if (!LaunchBlocks(st, io, plan)) return false;
    if (!AECM_HIP_OK(hipEventRecord(ev_stop_[slot], stream_))) return false;
    ++timer_pending_;
    return true;
}

bool BatchEngine::ProcessBlocksHost(const IoView &io, int num_blocks) {
    if (switches_.trace) return false;                // the block trace is for device-pointer launches (the C ABI answers AECM_UNSUPPORTED_FUNCTION_ERROR)
    if (!AECM_HIP_OK(hipSetDevice(device_))) return false;
    // Dense repack on the device side: [S][T*64] for each of far / near / (clean) / out.
    const size_t per = (size_t)num_streams_ * num_blocks * kBlock;
    const int n_in = io.near_clean ? 3 : 2;
    const size_t need = per * (n_in + 1);
#if defined(AECM_EXPERIMENTS)
    static const bool mapped = [] { const char *e = getenv("AECM_HOST_MAPPED"); return !(e && e[0] == '0'); }();
#else
    constexpr bool mapped = true;
#endif
    if (mapped && need * sizeof(int16_t) <= kMappedBytes) return ProcessBlocksHostMapped(io, num_blocks);
    if (need > stage_elems_) {
        (void)hipFree(stage_dev_);
        stage_dev_ = nullptr;
        stage_elems_ = 0;
        if (!AECM_HIP_OK(hipMalloc((void **)&stage_dev_, need * sizeof(int16_t)))) return false;
        stage_elems_ = need;
    }
    const bool dense = io.block_stride == kBlock && io.stream_stride == (int64_t)num_blocks * kBlock;
#if defined(AECM_EXPERIMENTS)
    static const bool pipeline = [] { const char *e = getenv("AECM_HOST_PIPELINE"); return !(e && e[0] == '0'); }();
#else
    constexpr bool pipeline = true;
#endif
    if (pipeline && dense && num_streams_ >= 2 * kHostChunkStreams) return ProcessBlocksHostPipelined(io, num_blocks);
    std::vector<int16_t> tmp;
    auto upload = [&](const int16_t *src, int16_t *dst) -> bool {
        if (dense) return AECM_HIP_OK(hipMemcpyAsync(dst, src, per * sizeof(int16_t), hipMemcpyHostToDevice, stream_));
        tmp.resize(per);
        for (int s = 0; s < num_streams_; ++s)
            for (int b = 0; b < num_blocks; ++b)
                memcpy(&tmp[((size_t)s * num_blocks + b) * kBlock], src + s * io.stream_stride + b * io.block_stride,
                       kBlock * sizeof(int16_t));
        return AECM_HIP_OK(hipMemcpy(dst, tmp.data(), per * sizeof(int16_t), hipMemcpyHostToDevice));
    };
    IoView dev;
    dev.far = stage_dev_;
    dev.near = stage_dev_ + per;
    dev.near_clean = io.near_clean ? stage_dev_ + 2 * per : nullptr;
    dev.out = stage_dev_ + (size_t)n_in * per;
    dev.stream_stride = (int64_t)num_blocks * kBlock;
    dev.block_stride = kBlock;
    if (!upload(io.far, const_cast<int16_t *>(dev.far))) return false;
    if (!upload(io.near, const_cast<int16_t *>(dev.near))) return false;
    if (io.near_clean && !upload(io.near_clean, const_cast<int16_t *>(dev.near_clean))) return false;
    if (!ProcessBlocks(dev, num_blocks)) return false;
    if (dense) {
        if (!AECM_HIP_OK(hipMemcpyAsync(io.out, dev.out, per * sizeof(int16_t), hipMemcpyDeviceToHost, stream_))) return false;
        return Drain();
    }
    tmp.resize(per);
    if (!AECM_HIP_OK(hipMemcpyAsync(tmp.data(), dev.out, per * sizeof(int16_t), hipMemcpyDeviceToHost, stream_))) return false;
    if (!Drain()) return false;
    for (int s = 0; s < num_streams_; ++s)
        for (int b = 0; b < num_blocks; ++b)
            memcpy(io.out + s * io.stream_stride + b * io.block_stride, &tmp[((size_t)s * num_blocks + b) * kBlock],
                   kBlock * sizeof(int16_t));
    return true;
}

bool BatchEngine::ProcessBlocksHostMapped(const IoView &io, int num_blocks) {
    if (!mapped_host_) {                          // both pointers are published together, only when both calls succeeded
        void *dev = nullptr;
        int16_t *host = nullptr;
        if (!AECM_HIP_OK(hipHostMalloc((void **)&host, kMappedBytes, hipHostMallocMapped))) return false;
        if (!AECM_HIP_OK(hipHostGetDevicePointer(&dev, host, 0)) || !dev) {
            (void)hipHostFree(host);
            return false;
        }
        mapped_host_ = host;
        mapped_dev_ = static_cast<int16_t *>(dev);
    }
    const RowLayout rows{num_streams_, num_blocks, io.stream_stride, io.block_stride};
    const bool has_clean = io.near_clean != nullptr;
    const IoView ours = StagedIo(mapped_host_, rows.row(), rows.per(), has_clean);      // the same planes as the host and as the device see them
    const IoView dev = StagedIo(mapped_dev_, rows.row(), rows.per(), has_clean);
    PackRows(rows, io.far, const_cast<int16_t *>(ours.far));
    PackRows(rows, io.near, const_cast<int16_t *>(ours.near));
    if (has_clean) PackRows(rows, io.near_clean, const_cast<int16_t *>(ours.near_clean));
    if (!LaunchBlocks(st_, dev, PlanLaunch(policy_, switches_, num_streams_, num_blocks, has_clean))) return false;
    if (!Drain()) return false;
    UnpackRows(rows, ours.out, io.out);
    return true;
}

// Dense host buffers, many streams: the streams are cut into chunks; a helper thread downloads chunk k
// (pageable-memory copies block their host thread) while this thread uploads and launches chunk k + 1,
// so both directions of the link are busy.
bool BatchEngine::ProcessBlocksHostPipelined(const IoView &io, int num_blocks) {
    const size_t row = (size_t)num_blocks * kBlock;                       // samples per stream
    const bool has_clean = io.near_clean != nullptr;
    const size_t per = (size_t)num_streams_ * row;
    if (!download_stream_ && !AECM_HIP_OK(hipStreamCreateWithFlags(&download_stream_, hipStreamNonBlocking))) return false;
    if (!FlushTimers()) return false;
    const int n_chunks = (num_streams_ + kHostChunkStreams - 1) / kHostChunkStreams;
    std::vector<hipEvent_t> done(n_chunks, nullptr);
    bool ok = true;
    for (auto &e : done) ok = ok && AECM_HIP_OK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    const int16_t *dout = StagedIo(stage_dev_, row, per, has_clean).out;
    std::atomic<int> launched{0};
    std::atomic<bool> failed{!ok};
    std::thread downloader([&] {
        if (!AECM_HIP_OK(hipSetDevice(device_))) { failed = true; return; }
        for (int k = 0; k < n_chunks; ++k) {
            while (launched.load(std::memory_order_acquire) <= k) {
                if (failed.load()) return;
                std::this_thread::yield();
            }
            const size_t first = (size_t)k * kHostChunkStreams;
            const size_t count = std::min<size_t>(kHostChunkStreams, num_streams_ - first);
            if (!AECM_HIP_OK(hipEventSynchronize(done[k])) ||
                !AECM_HIP_OK(hipMemcpyAsync(io.out + first * row, dout + first * row, count * row * sizeof(int16_t),
                                            hipMemcpyDeviceToHost, download_stream_)) ||
                !AECM_HIP_OK(hipStreamSynchronize(download_stream_))) {
                failed = true;
                return;
            }
        }
    });
    for (int k = 0; k < n_chunks && !failed.load(); ++k) {
        const size_t first = (size_t)k * kHostChunkStreams;
        const size_t count = std::min<size_t>(kHostChunkStreams, num_streams_ - first);
        const size_t off = first * row, bytes = count * row * sizeof(int16_t);
        const IoView dev = StagedIo(stage_dev_ + off, row, per, has_clean);      // the chunk's streams in the batch's planes
        auto upload = [&](const int16_t *src, const int16_t *dst) {
            return AECM_HIP_OK(hipMemcpyAsync(const_cast<int16_t *>(dst), src + off, bytes, hipMemcpyHostToDevice, stream_));
        };
        const bool up = upload(io.far, dev.far) && upload(io.near, dev.near) && (!has_clean || upload(io.near_clean, dev.near_clean)) &&
                        LaunchBlocks(OffsetToStream(st_, first), dev, PlanLaunch(policy_, switches_, (int)count, num_blocks, has_clean)) &&
                        AECM_HIP_OK(hipEventRecord(done[k], stream_));
        if (!up) failed = true;
        launched.store(k + 1, std::memory_order_release);
    }
    if (failed.load()) launched.store(n_chunks, std::memory_order_release);      // let the helper fall out of its wait
    downloader.join();
    ok = !failed.load() && Drain();
    for (auto e : done)
        if (e) (void)hipEventDestroy(e);
    return ok;
}

// Grow-only device scratch shared by the recording batches (no hipMalloc / hipFree per call).
bool BatchEngine::EnsureRecordingScratch(size_t map_elems, size_t sample_elems) {
    return GrowDeviceBuffer((void **)&rec_maps_, &rec_maps_elems_, map_elems, sizeof(int32_t), stream_) &&
           GrowDeviceBuffer((void **)&rec_scratch_, &rec_scratch_elems_, sample_elems, sizeof(int16_t), stream_);
}

bool BatchEngine::ProcessRecordings(const int16_t *far, const int16_t *near, const int16_t *clean, int16_t *out,
                                    int64_t stream_stride, int frame, int n_calls, int16_t ms, bool host_pointers, int32_t *rc) {
    return ProcessRecordingsRagged(far, near, clean, out, stream_stride, frame, n_calls, nullptr, ms, host_pointers, rc, nullptr);
}

// calls (may be null: every stream makes n_calls calls): the schedule of a session of k calls is the prefix of the schedule of n_calls
// calls, so stream s runs the first blocks_after_call[calls[s] - 1] blocks of the common schedule (a ragged launch) and its
// output is assembled up to calls[s] * frame samples, zeros behind.  The gathers stay full-width.
bool BatchEngine::ProcessRecordingsRagged(const int16_t *far, const int16_t *near, const int16_t *clean, int16_t *out, int64_t stream_stride,
                                          int frame, int n_calls, const int32_t *calls, int16_t ms, bool host_pointers, int32_t *rc,
                                          int32_t *codes) {
    if (!AECM_HIP_OK(hipSetDevice(device_))) return false;
    if (switches_.trace) { *rc = kErrUnsupported; return true; }     // the recording's call-to-block map is not block-aligned: no block trace of it
    if (mixed_rates_) { *rc = kErrUnsupported; return true; }        // an imported stream runs at another rate than fs_
    const RecordingSchedule sch = BuildRecordingSchedule(fs_, frame, n_calls, ms);
    std::vector<int32_t> lens, limits;                                // per stream: blocks to run, output samples to assemble
    if (calls) {
        if ((int)sch.blocks_after_call.size() != n_calls) {           // the session could not even be initialised: every call returns that
            *rc = sch.first_error;
            for (int s = 0; codes && s < num_streams_; ++s) codes[s] = calls[s] > 0 ? sch.first_error : 0;
            return true;
        }
        *rc = 0;
        lens.resize(num_streams_);
        limits.resize(num_streams_);
        for (int s = 0; s < num_streams_; ++s) {
            const int k = calls[s];
            lens[s] = k > 0 ? sch.blocks_after_call[k - 1] : 0;
            limits[s] = k * frame;
            const int32_t code = k > 0 ? sch.code_after_call[k - 1] : 0;
            if (codes) codes[s] = code;
            if (*rc == 0) *rc = code;
            // a session one of whose calls failed (not the 12100 warning) is not run at all: its row is written as zeros and its
            // state stays as it was; the sessions that end before the failing call run as usual
            if (code != 0 && code != kWarnBadParameter) lens[s] = limits[s] = 0;
        }
    } else {
        if (sch.first_error) { *rc = sch.first_error; return true; }
        *rc = sch.warned ? kWarnBadParameter : 0;
    }
    const int64_t n_in = (int64_t)n_calls * frame, n_blk = (int64_t)sch.n_blocks * kBlock;
    const int n_near = clean ? 2 : 1;      // the clean near-end follows the near-end's schedule sample for sample
    // Device scratch per stream: gathered far/near(/clean) blocks + block outputs (+ staged I/O for host pointers).
    // The streams are processed in chunks so that the scratch stays below kRecordingScratchBytes whatever the
    // batch size and recording length (and the 1-D grids of the gather kernels stay below 2^31 workgroups).
    const size_t blk_per_stream = (size_t)(2 + n_near) * (size_t)n_blk;
    const size_t io_per_stream = host_pointers ? (size_t)(2 + n_near) * (size_t)n_in : 0;
    const size_t per_stream = std::max<size_t>(blk_per_stream + io_per_stream, 1);
    const int64_t tiles = std::max<int64_t>((std::max(n_in, n_blk) + 255) / 256, 1);
    int64_t chunk = std::max<int64_t>((int64_t)(kRecordingScratchBytes / (per_stream * sizeof(int16_t))), 1);
    chunk = std::min<int64_t>(chunk, 0x7fffffffll / tiles);
    chunk = std::min<int64_t>(chunk, num_streams_);
    const size_t map_elems = std::max<size_t>((size_t)(2 * n_blk + n_in), 1);
    if (!EnsureRecordingScratch(map_elems + (calls ? (size_t)num_streams_ : 0), (size_t)chunk * per_stream)) return false;
    int32_t *maps = rec_maps_;
    int32_t *limits_dev = calls ? rec_maps_ + map_elems : nullptr;
    bool ok = true;
    if (calls) ok = AECM_HIP_OK(hipMemcpyAsync(limits_dev, limits.data(), limits.size() * sizeof(int32_t), hipMemcpyHostToDevice, stream_));
    if (ok && n_blk > 0) {
        ok = AECM_HIP_OK(hipMemcpyAsync(maps, sch.far_map.data(), n_blk * sizeof(int32_t), hipMemcpyHostToDevice, stream_)) &&
             AECM_HIP_OK(hipMemcpyAsync(maps + n_blk, sch.near_map.data(), n_blk * sizeof(int32_t), hipMemcpyHostToDevice, stream_));
    }
    if (ok) ok = AECM_HIP_OK(hipMemcpyAsync(maps + 2 * n_blk, sch.out_map.data(), n_in * sizeof(int32_t), hipMemcpyHostToDevice, stream_));
    for (int64_t s0 = 0; ok && s0 < num_streams_; s0 += chunk) {
        const size_t C = (size_t)std::min<int64_t>(chunk, num_streams_ - s0);
        int16_t *bfar = rec_scratch_, *bnear = bfar + C * n_blk, *bout = bnear + C * n_blk, *bclean = bout + C * n_blk;
        const int16_t *dfar = far + s0 * stream_stride, *dnear = near + s0 * stream_stride;
        const int16_t *dclean = clean ? clean + s0 * stream_stride : nullptr;
        int16_t *dout = out + s0 * stream_stride;
        int64_t dstride = stream_stride;
        if (host_pointers) {
            int16_t *io = rec_scratch_ + C * blk_per_stream;
            dstride = n_in;
            auto upload = [&](const int16_t *src, int16_t *dst) {
                return AECM_HIP_OK(hipMemcpy2DAsync(dst, n_in * 2, src, stream_stride * 2, n_in * 2, C, hipMemcpyHostToDevice, stream_));
            };
            ok = upload(dfar, io) && upload(dnear, io + C * n_in) && (!clean || upload(dclean, io + 3 * C * n_in));
            dfar = io;
            dnear = io + C * n_in;
            dout = io + 2 * C * n_in;
            if (clean) dclean = io + 3 * C * n_in;
        }
        if (ok && n_blk > 0) {
            ok = AECM_HIP_OK(LaunchGatherByMap(dfar, dstride, maps, n_blk, bfar, n_blk, (int)C, stream_)) &&
                 AECM_HIP_OK(LaunchGatherByMap(dnear, dstride, maps + n_blk, n_blk, bnear, n_blk, (int)C, stream_)) &&
                 (!clean || AECM_HIP_OK(LaunchGatherByMap(dclean, dstride, maps + n_blk, n_blk, bclean, n_blk, (int)C, stream_)));
            if (ok) {
                IoView io{bfar, bnear, clean ? bclean : nullptr, bout, n_blk, kBlock};
                ok = calls ? ProcessBlocksRaggedRange(io, sch.n_blocks, (int)s0, (int)C, lens.data() + s0) == 0
                           : ProcessBlocksRange(io, sch.n_blocks, (int)s0, (int)C);
            }
        }
        // pass-through samples of the start-up phase come from the clean near-end when there is one
        // (reference echo_control_mobile.cc:285-291)
        if (ok) ok = AECM_HIP_OK(LaunchAssembleOutput(bout, n_blk, clean ? dclean : dnear, dstride, maps + 2 * n_blk, n_in, dout, dstride,
                                                      (int)C, stream_, calls ? limits_dev + s0 : nullptr));
        if (ok && host_pointers)
            ok = AECM_HIP_OK(hipMemcpy2DAsync(out + s0 * stream_stride, stream_stride * 2, dout, n_in * 2, n_in * 2, C,
                                              hipMemcpyDeviceToHost, stream_));
    }
    if (!Drain()) ok = false;      // sch (the maps' host copy) goes out of scope
    return ok;
}

bool BatchEngine::Synchronize() {
    if (!AECM_HIP_OK(hipSetDevice(device_))) return false;
    return Drain();
}

bool BatchEngine::LastLaunchMs(float *ms) {
    if (!FlushTimers()) return false;
    *ms = last_ms_;
    return true;
}

bool BatchEngine::Timers(double *total_ms, int64_t *launches) {
    if (!FlushTimers()) return false;
    *total_ms = total_ms_;
    *launches = launches_;
    return true;
}

void BatchEngine::ResetTimers() {
    (void)FlushTimers();
    total_ms_ = 0.0;
    launches_ = 0;
}

bool BatchEngine::SetEchoPath(int stream, const int16_t path[kBins]) {
    if (stream < 0 || stream >= num_streams_) return false;
    if (!AECM_HIP_OK(hipSetDevice(device_))) return false;
    // WebRtcAecm_InitEchoPathCore touches the two channel words of the lane-vector image and seven scalars: write
    // exactly those (two 256-byte rows + one scalar patch), in stream order after whatever is still running.
    std::vector<uint32_t> vec(kVecWordsPerStream, 0u);
    int32_t scal[kNumScal] = {0};
    aecm::SetEchoPath(vec.data(), scal, path);
    uint32_t *dvec = st_.vec + (size_t)stream * kVecWordsPerStream;
    // `vec` is a local: whatever happens below, no copy from it may still be in flight when this function returns
    bool ok = AECM_HIP_OK(hipMemcpyAsync(dvec + V_CH16 * kLanes, vec.data() + V_CH16 * kLanes, kLanes * sizeof(uint32_t), hipMemcpyHostToDevice, stream_)) &&
              AECM_HIP_OK(hipMemcpyAsync(dvec + V_CH32 * kLanes, vec.data() + V_CH32 * kLanes, kLanes * sizeof(uint32_t), hipMemcpyHostToDevice, stream_));
    if (ok) {
        const int32_t fields[7] = {S_B64_CHSTORED, S_B64_CHADAPT16, S_B64_CHADAPT32, S_MSE_ADAPT_OLD, S_MSE_STORED_OLD, S_MSE_THRESH, S_MSECNT};
        int32_t values[7];
        for (int i = 0; i < 7; ++i) values[i] = scal[fields[i]];
        ok = PatchScalars(fields, values, 7, stream, 1);
    }
    const bool drained = Drain();
    return ok && drained;
}

bool BatchEngine::GetEchoPath(int stream, int16_t path[kBins]) {
    if (stream < 0 || stream >= num_streams_) return false;
    if (!AECM_HIP_OK(hipSetDevice(device_))) return false;
    std::vector<uint32_t> ch(kLanes);
    std::vector<int32_t> scal(kNumScal);
    if (!Drain()) return false;
    if (!AECM_HIP_OK(hipMemcpy(ch.data(), st_.vec + (size_t)stream * kVecWordsPerStream + V_CH16 * kLanes,
                               kLanes * sizeof(uint32_t), hipMemcpyDeviceToHost)))
        return false;
    if (!AECM_HIP_OK(hipMemcpy(scal.data(), st_.scal + (size_t)stream * kNumScal, kNumScal * sizeof(int32_t),
                               hipMemcpyDeviceToHost)))
        return false;
    for (int t = 0; t < kLanes; ++t) path[t] = (int16_t)(ch[t] & 0xffff);
    path[64] = (int16_t)scal[S_B64_CHSTORED];
    return true;
}

// Snapshot = header + vec + scal + hist (aecm_state_check.h: SnapshotHeader).  The header pins the layout the blob was written
// with, so a blob from another build (different field lists) or a corrupted one is refused instead of being used as addresses.
static_assert(kStateHeaderBytes == BatchEngine::kStateHeaderBytes && kStateBlobBytes == BatchEngine::kStateBytes, "snapshot blob size");

bool BatchEngine::ExportState(int stream, void *buf) {
    if (stream < 0 || stream >= num_streams_) return false;
    if (!AECM_HIP_OK(hipSetDevice(device_)) || !Drain()) return false;
    uint8_t *p = static_cast<uint8_t *>(buf);
    uint8_t *body = p + kStateHeaderBytes;
    if (!(AECM_HIP_OK(hipMemcpy(body, st_.vec + (size_t)stream * kVecWordsPerStream, kVecWordsPerStream * 4, hipMemcpyDeviceToHost)) &&
          AECM_HIP_OK(hipMemcpy(body + kVecWordsPerStream * 4, st_.scal + (size_t)stream * kNumScal, kNumScal * 4, hipMemcpyDeviceToHost)) &&
          AECM_HIP_OK(hipMemcpy(body + kVecWordsPerStream * 4 + kNumScal * 4, st_.hist + (size_t)stream * kHistWordsPerStream,
                                kHistWordsPerStream * 2, hipMemcpyDeviceToHost))))
        return false;
    int32_t mult = 0;
    memcpy(&mult, body + kVecWordsPerStream * 4 + S_MULT * 4, 4);
    const SnapshotHeader h{kSnapshotMagic, kStateLayoutVersion, (uint32_t)mult * 8000u, (uint32_t)kNumVec, (uint32_t)kNumScal,
                           (uint32_t)kHistory, (uint32_t)kLanes, 0u};
    memcpy(p, &h, sizeof h);
    return true;
}

// 0, kErrBadParameter (not a snapshot of this layout, or index-like fields out of range) or kErrUnspecified (HIP).
int32_t BatchEngine::ImportState(int stream, const void *buf) {
    if (stream < 0 || stream >= num_streams_) return kErrBadParameter;
    const uint8_t *p = static_cast<const uint8_t *>(buf);
    SnapshotHeader h;
    memcpy(&h, p, sizeof h);
    if (!SnapshotHeaderOk(h)) return kErrBadParameter;
    const uint8_t *body = p + kStateHeaderBytes;
    int32_t scal[kNumScal];
    memcpy(scal, body + kVecWordsPerStream * 4, sizeof scal);
    // everything the kernel uses as an index or a shift count, and the value ranges its arithmetic shortcuts rely on
    std::vector<uint32_t> vec(kVecWordsPerStream);
    memcpy(vec.data(), body, kVecWordsPerStream * 4);
    const bool sane = ValidateStateImage(vec.data(), scal, (int)h.fs) == nullptr;
    if (!sane) return kErrBadParameter;
    if (!AECM_HIP_OK(hipSetDevice(device_)) || !Drain()) return kErrUnspecified;
    if (!(AECM_HIP_OK(hipMemcpy(st_.vec + (size_t)stream * kVecWordsPerStream, body, kVecWordsPerStream * 4, hipMemcpyHostToDevice)) &&
          AECM_HIP_OK(hipMemcpy(st_.scal + (size_t)stream * kNumScal, body + kVecWordsPerStream * 4, kNumScal * 4, hipMemcpyHostToDevice)) &&
          AECM_HIP_OK(hipMemcpy(st_.hist + (size_t)stream * kHistWordsPerStream, body + kVecWordsPerStream * 4 + kNumScal * 4,
                                kHistWordsPerStream * 2, hipMemcpyHostToDevice))))
        return kErrUnspecified;
    if ((int)h.fs != fs_) mixed_rates_ = true;       // ProcessRecordings schedules every stream for fs_: refuse until the next Init
    return 0;
}

bool BatchEngine::EnsureStateStage(int streams) {
    const size_t need = (size_t)std::min(streams, kStateStageStreams) * kStateBytes;
    if (need > state_stage_bytes_) {
        if (!AECM_HIP_OK(hipStreamSynchronize(stream_))) return false;
        (void)hipFree(state_stage_);
        state_stage_ = nullptr;
        state_stage_bytes_ = 0;
        if (!AECM_HIP_OK(hipMalloc((void **)&state_stage_, need))) return false;
        state_stage_bytes_ = need;
    }
    return state_verdict_ || AECM_HIP_OK(hipMalloc((void **)&state_verdict_, 2 * sizeof(uint32_t)));
}

bool BatchEngine::ExportStates(int first, int count, void *states, bool device) {
    if (first < 0 || count < 0 || first + count > num_streams_) return false;
    if (!AECM_HIP_OK(hipSetDevice(device_))) return false;
    if (count == 0) return Drain();
    if (device) return AECM_HIP_OK(LaunchGatherStates(st_, first, count, states, stream_)) && Drain();
    if (!EnsureStateStage(count)) return false;
    uint8_t *dst = static_cast<uint8_t *>(states);
    for (int s0 = 0; s0 < count; s0 += kStateStageStreams) {                      // the copy of a chunk is ordered before the next gather
        const int n = std::min(kStateStageStreams, count - s0);
        if (!AECM_HIP_OK(LaunchGatherStates(st_, first + s0, n, state_stage_, stream_)) ||
            !AECM_HIP_OK(hipMemcpyAsync(dst + (size_t)s0 * kStateBytes, state_stage_, (size_t)n * kStateBytes, hipMemcpyDeviceToHost, stream_)))
            return false;
    }
    return Drain();
}

int32_t BatchEngine::ImportStates(int first, int count, const void *states, bool device) {
    if (first < 0 || count < 0 || first + count > num_streams_) return kErrBadParameter;
    if (!AECM_HIP_OK(hipSetDevice(device_))) return kErrUnspecified;
    if (count == 0) return 0;
    bool other_rate = false;
    if (device) {
        // the kernels read the blobs as 32-bit words: a pointer that is not a multiple of 4 would fault on the GPU
        if (reinterpret_cast<uintptr_t>(states) & 3) return kErrBadParameter;
        if (!EnsureStateStage(1)) return kErrUnspecified;
        const uint32_t preset[2] = {0xffffffffu, 0u};
        uint32_t verdict[2] = {0, 0};
        if (!AECM_HIP_OK(hipMemcpyAsync(state_verdict_, preset, sizeof preset, hipMemcpyHostToDevice, stream_)) ||
            !AECM_HIP_OK(LaunchValidateStates(states, count, fs_, state_verdict_, stream_)) ||
            !AECM_HIP_OK(hipMemcpyAsync(verdict, state_verdict_, sizeof verdict, hipMemcpyDeviceToHost, stream_)) || !Drain())
            return kErrUnspecified;
        if (verdict[0] != 0xffffffffu) return kErrBadParameter;
        other_rate = verdict[1] != 0;
        if (!AECM_HIP_OK(LaunchScatterStates(st_, first, count, states, stream_)) || !Drain()) return kErrUnspecified;
    } else {
        const uint8_t *src = static_cast<const uint8_t *>(states);
        for (int s = 0; s < count; ++s) {                                        // all or nothing: every blob before any stream
            const uint8_t *blob = src + (size_t)s * kStateBytes;
            SnapshotHeader h;
            memcpy(&h, blob, sizeof h);
            if (!SnapshotHeaderOk(h)) return kErrBadParameter;
            const uint32_t *vec = reinterpret_cast<const uint32_t *>(blob + kStateHeaderBytes);      // blobs are 16-byte multiples: aligned if the buffer is
            const int32_t *scal = reinterpret_cast<const int32_t *>(blob + kStateHeaderBytes + kVecWordsPerStream * 4);
            uint32_t vec_copy[kVecWordsPerStream];
            int32_t scal_copy[kNumScal];
            if (reinterpret_cast<uintptr_t>(blob) & 3) {
                memcpy(vec_copy, vec, sizeof vec_copy);
                memcpy(scal_copy, scal, sizeof scal_copy);
                vec = vec_copy;
                scal = scal_copy;
            }
            if (ValidateStateImage(vec, scal, (int)h.fs) != nullptr) return kErrBadParameter;
            other_rate = other_rate || (int)h.fs != fs_;
        }
        if (!EnsureStateStage(count)) return kErrUnspecified;
        for (int s0 = 0; s0 < count; s0 += kStateStageStreams) {
            const int n = std::min(kStateStageStreams, count - s0);
            if (!AECM_HIP_OK(hipMemcpyAsync(state_stage_, src + (size_t)s0 * kStateBytes, (size_t)n * kStateBytes, hipMemcpyHostToDevice, stream_)) ||
                !AECM_HIP_OK(LaunchScatterStates(st_, first + s0, n, state_stage_, stream_)))
                return kErrUnspecified;
        }
        if (!Drain()) return kErrUnspecified;
    }
    if (other_rate) mixed_rates_ = true;
    return 0;
}

bool BatchEngine::Digest(int stream, uint32_t digest[kDigestWords]) {
    if (stream < 0 || stream >= num_streams_) return false;
    if (!AECM_HIP_OK(hipSetDevice(device_))) return false;
    std::vector<uint32_t> vec(kVecWordsPerStream);
    std::vector<int32_t> scal(kNumScal);
    std::vector<uint16_t> hist(kHistWordsPerStream);
    if (!Drain()) return false;
    if (!AECM_HIP_OK(hipMemcpy(vec.data(), st_.vec + (size_t)stream * kVecWordsPerStream, vec.size() * sizeof(uint32_t),
                               hipMemcpyDeviceToHost)))
        return false;
    if (!AECM_HIP_OK(hipMemcpy(scal.data(), st_.scal + (size_t)stream * kNumScal, scal.size() * sizeof(int32_t),
                               hipMemcpyDeviceToHost)))
        return false;
    if (!AECM_HIP_OK(hipMemcpy(hist.data(), st_.hist + (size_t)stream * kHistWordsPerStream,
                               hist.size() * sizeof(uint16_t), hipMemcpyDeviceToHost)))
        return false;
    ComputeDigest(vec.data(), scal.data(), hist.data(), digest);
    return true;
}

}  // namespace aecm
