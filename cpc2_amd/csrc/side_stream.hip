// The library's side stream: ONE stream per device, created on first use beside the caller's, for work that nothing on the
// caller's stream needs -- the criterion's reference lists and deferred backward (infonce.hip, with events of its own) and the
// parameter-gradient "tails" of the encoder, the recurrent cells and the transformer (side_tail_*).  Everything queued on it runs
// in queue order.  Host code only: no kernel is launched here.
#include "common.h"

#include <map>
#include <mutex>

namespace cpc {

namespace {

struct SideStream {
    hipStream_t stream = nullptr;
    hipEvent_t tail_fork = nullptr, tail = nullptr;     // side_tail_*: work of a backward entry point finishing on this stream
    bool tail_pending = false;
};

// caller == nullptr: the record must exist already (nothing to create a stream apart from)
int side_record(SideStream **out, const hipStream_t *caller)
{
    static std::mutex mu;
    static std::map<int, SideStream> sides;
    int dev = 0;
    CPC_CHECK_HIP(hipGetDevice(&dev));
    std::lock_guard<std::mutex> lk(mu);
    if (caller == nullptr) {
        const auto it = sides.find(dev);
        CPC_REQUIRE(it != sides.end() && it->second.stream != nullptr, "side_tail_end: no side_tail_begin ran on device %d", dev);
        *out = &it->second;
        return CPC_OK;
    }
    SideStream &sd = sides[dev];
    if (sd.stream == nullptr) {
        // DEFAULT priority, deliberately.  A lowest-priority stream looked right for work that runs beside the caller's, and costs
        // nothing in a single-process run -- but in a process that has also initialised RCCL every kernel of the step ran ~45 %
        // slower (7.7 against 5.3 ms per step with one rank; found by bisection, profiles/r03_dist_priority_bisect.txt).
        // ... and on a hardware queue of its own: tested against the caller's stream (stream_create_apart, rowops.hip)
        CPC_TRY(stream_create_apart(caller, 1, &sd.stream));
        CPC_CHECK_HIP(hipEventCreateWithFlags(&sd.tail_fork, hipEventDisableTiming));
        CPC_CHECK_HIP(hipEventCreateWithFlags(&sd.tail, hipEventDisableTiming));
    }
    *out = &sd;
    return CPC_OK;
}

}  // namespace

int side_stream_get(hipStream_t caller, hipStream_t *out)
{
    SideStream *side = nullptr;
    CPC_TRY(side_record(&side, &caller));
    *out = side->stream;
    return CPC_OK;
}

// ---- "tail" work of a backward entry point on the library's side stream: ordered behind what `st` holds now (and behind whatever
// the side stream already has queued); whoever reads its results waits at side_tail_join
int side_tail_begin(hipStream_t st, hipStream_t *side_stream)
{
    SideStream *side = nullptr;
    CPC_TRY(side_record(&side, &st));
    CPC_CHECK_HIP(hipEventRecord(side->tail_fork, st));
    CPC_CHECK_HIP(hipStreamWaitEvent(side->stream, side->tail_fork, 0));
    *side_stream = side->stream;
    return CPC_OK;
}
int side_tail_end()
{
    SideStream *side = nullptr;
    CPC_TRY(side_record(&side, nullptr));
    CPC_CHECK_HIP(hipEventRecord(side->tail, side->stream));
    side->tail_pending = true;
    return CPC_OK;
}
int side_tail_join(hipStream_t st)
{
    SideStream *side = nullptr;
    CPC_TRY(side_record(&side, &st));
    if (side->tail_pending) {
        ProfScope held(PROF_SIDE_WAIT, st);          // (bench.py: how long `st` stands still here)
        CPC_CHECK_HIP(hipStreamWaitEvent(st, side->tail, 0));
        side->tail_pending = false;
    }
    return CPC_OK;
}

// the same wait WITHOUT taking the tail off the books: a helper stream (the data-parallel exchange's) orders itself behind the tail
// while the caller's stream goes on; whoever reuses the tail's buffers still joins with side_tail_join
int side_tail_wait(hipStream_t st)
{
    SideStream *side = nullptr;
    CPC_TRY(side_record(&side, &st));
    if (side->tail_pending) CPC_CHECK_HIP(hipStreamWaitEvent(st, side->tail, 0));
    return CPC_OK;
}

}  // namespace cpc

extern "C" int cpc_side_stream(cpc_stream_t caller, cpc_stream_t *out)
{
    CPC_REQUIRE(out != nullptr, "cpc_side_stream: null output");
    hipStream_t st = nullptr;
    CPC_TRY(cpc::side_stream_get(static_cast<hipStream_t>(caller), &st));
    *out = st;
    return CPC_OK;
}

extern "C" int cpc_side_tail_join(cpc_stream_t stream) { return cpc::side_tail_join(static_cast<hipStream_t>(stream)); }
extern "C" int cpc_side_tail_wait(cpc_stream_t stream) { return cpc::side_tail_wait(static_cast<hipStream_t>(stream)); }
