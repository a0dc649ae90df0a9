// Stage clock of one execution lane, for roofline accounting: HIP events on the lane's own stream around every launch while
// profiling is on, nothing but the launch while it is off.  Contract: every method is called under the lane's mutex (the
// clock has no lock of its own); the stream outlives the clock's last use; events come from a pool of the clock's own and
// are read back -- with a wait for the stream -- by take_stats(), set_profiling() or after 8192 launches.
// ST_GEMM is the sum over all GEMM launches of the encoder; ST_GEMM_* split the same launches by kernel flavour (what
// the by-grid table of a kernel trace tells apart): residual-stream writers with row statistics (patch / proj / fc2),
// LayerNorm-folded consumers without / with GELU (qkv / fc1), everything else (neck).
#pragma once

#include "common.hpp"

namespace dlimg {

enum Stage { ST_PRE = 0, ST_GEMM, ST_LAYERNORM, ST_ATTN_WINDOW, ST_ATTN_GLOBAL, ST_ENC_OTHER, ST_DECODER, ST_POST,
             ST_GEMM_STATS, ST_GEMM_NORM, ST_GEMM_NORM_GELU, ST_GEMM_OTHER,
             // r06: the stream writers (ST_GEMM_STATS) once more by shape -- they share a kernel and a grid, so no profiler
             // table can tell them apart, and proj (K = D: 152 FLOP per byte at ViT-B) sits on the other side of the ridge
             // from fc2 (K = 4 D)
             ST_GEMM_PATCH, ST_GEMM_PROJ, ST_GEMM_FC2, ST_COUNT };

struct StageStats {
    double ms[ST_COUNT] = {0};
    double work[ST_COUNT] = {0};     // algorithmic FLOPs (MFMA stages) or bytes (HBM stages)
    long launches[ST_COUNT] = {0};
};

class StageClock {
  public:
    explicit StageClock(hipStream_t stream) : stream_(stream) {}
    ~StageClock();
    StageClock(StageClock const&) = delete;
    StageClock& operator=(StageClock const&) = delete;

    bool profiling() const { return profiling_; }
    void set_profiling(bool on);
    StageStats take_stats();

    // launches: kernel launches inside `launch` (one event pair around all of them)
    template <typename F> void timed(Stage st, double work, F&& launch, int launches = 1) {
        if (!profiling_) {
            launch();
            return;
        }
        Pending p = event_pair(st, work);
        p.launches = launches;
        HIP_CHECK(hipEventRecord(p.a, stream_));
        launch();
        HIP_CHECK(hipEventRecord(p.b, stream_));
        add(p);
    }
    // For a launch that takes its own time (events attached to the dispatch, kernels.hpp: gemm): the pair to hand to it,
    // and add() once it has been enqueued.  The time also counts for the stages `also` and `shape` (ST_COUNT: none).
    struct Pending { hipEvent_t a, b; Stage st; double work; Stage also = ST_COUNT; Stage shape = ST_COUNT; int launches = 1; };
    Pending event_pair(Stage st, double work, Stage also = ST_COUNT, Stage shape = ST_COUNT) {
        return Pending{take_event(), take_event(), st, work, also, shape};
    }
    void add(Pending const& p) {
        pending_.push_back(p);
        if (pending_.size() > 8192) flush_events();
    }

  private:
    void flush_events();
    hipEvent_t take_event();

    hipStream_t stream_;
    bool profiling_ = false;
    std::vector<Pending> pending_;
    std::vector<hipEvent_t> event_pool_;
    StageStats stats_;
};

}  // namespace dlimg
