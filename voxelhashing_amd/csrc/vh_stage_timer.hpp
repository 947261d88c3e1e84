// vh_stage_timer.hpp -- per-stage device timing with HIP events recorded on
// the stream the kernels are launched on (the reference's TimingLog,
// DSC/TimingLog.h:21-46, without its cudaDeviceSynchronize per stage).
#pragma once

#include <hip/hip_runtime.h>

#include "../../include/vh_api.h"
#include "../../include/vh_owners.hpp"

#include <cstdint>
#include <utility>
#include <vector>

struct VhStageTimer {
    explicit VhStageTimer(int nStages) : totalMs(nStages, 0.0), count(nStages, 0), open(nStages), pending(nStages) {}
    vh::Event get()
    {
        // timing only: a device-scope release event (a default event record idles the queue for ~6 us, which distorts
        // the frame rate being measured)
        if (pool.empty()) return vh::makeEvent(true);
        vh::Event e = std::move(pool.back());
        pool.pop_back();
        return e;
    }
    void start(int stage, hipStream_t s)
    {
        open[stage] = get();
        (void)hipEventRecord((hipEvent_t)open[stage].get(), s);
    }
    void stop(int stage, hipStream_t s)
    {
        vh::Event e = get();
        (void)hipEventRecord((hipEvent_t)e.get(), s);
        pending[stage].emplace_back(std::move(open[stage]), std::move(e));
    }
    // the NEXT kernel this thread launches (one of those that go through VH_LAUNCH_TIMED: the ray caster, computeNormals,
    // the fused integrate pass) is timed by its own dispatch time stamps: no record before or behind it
    void arm(int stage)
    {
        vh::Event a = get(), b = get();
        (void)vh_time_next_launch(a.get(), b.get());
        pending[stage].emplace_back(std::move(a), std::move(b));
    }
    // waits for the stream and folds all finished pairs into the totals
    void resolve(hipStream_t s)
    {
        (void)hipStreamSynchronize(s);
        for (size_t st = 0; st < pending.size(); st++) {
            for (auto& p : pending[st]) {
                float ms = 0.0f;
                if (hipEventElapsedTime(&ms, (hipEvent_t)p.first.get(), (hipEvent_t)p.second.get()) == hipSuccess) { totalMs[st] += ms; count[st]++; }
                pool.push_back(std::move(p.first));
                pool.push_back(std::move(p.second));
            }
            pending[st].clear();
        }
    }
    void clear()
    {
        for (size_t st = 0; st < totalMs.size(); st++) { totalMs[st] = 0.0; count[st] = 0; }
    }
    std::vector<double> totalMs;
    std::vector<uint64_t> count;
    std::vector<vh::Event> open;
    std::vector<std::vector<std::pair<vh::Event, vh::Event>>> pending;
    std::vector<vh::Event> pool;
};
