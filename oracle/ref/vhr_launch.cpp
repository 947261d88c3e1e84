/*
 * vhr_launch.cpp -- the workgroup scheduler of the launch emulator (include/cuda_runtime.h): a workgroup's threads as
 * cooperative fibers (ucontext), so that kernels with __syncthreads run serially on the CPU.
 *
 *   - The first thread (0, 0, 0) of every workgroup starts on a fiber.  If it returns without reaching a barrier,
 *     the other threads run one after the other on the caller's stack, as the emulator always did; a barrier-free
 *     kernel pays one fiber switch per workgroup and its results do not change.
 *   - If it stops at __syncthreads, every other thread starts on a fiber of its own and runs, in order z, y, x, until
 *     it reaches a barrier or returns.  When all of them wait at a barrier, all resume in the same order; when all
 *     have returned, the workgroup is done.
 *   - A barrier that only some threads reach (the others have returned), or one reached by a thread that runs
 *     without a fiber because the first thread returned without one, aborts with a message: CUDA leaves barriers in
 *     divergent code undefined, and the emulator will not pick a meaning for it.
 *
 * threadIdx is set before every resume.  Workgroups run one at a time, so __shared__ stays `static`.  Fiber stacks
 * have a guard page below them: an overflow faults instead of writing over a neighbour.
 */
#include "cuda_runtime.h"

#include <sys/mman.h>
#include <ucontext.h>
#include <unistd.h>

#include <vector>

namespace {

enum State { RUNNING, AT_BARRIER, DONE };

const size_t kStackBytes = 256 * 1024;

struct Fiber {
    ucontext_t ctx;
    char* stack = nullptr;  // the usable stack, above a guard page
    State state = DONE;
    uint3 tid;
};

struct Scheduler {
    std::vector<Fiber*> fibers;  // kept across launches: stacks are mapped once per thread
    ucontext_t main;
    Fiber* current = nullptr;    // the fiber running now, or nullptr when a thread runs on the caller's stack
    vhr_thread_fn fn = nullptr;
    void* arg = nullptr;
    size_t page = 0;

    Fiber* fiber(size_t i)
    {
        while (fibers.size() <= i) {
            if (!page) page = (size_t)sysconf(_SC_PAGESIZE);
            Fiber* f = new Fiber();
            void* m = mmap(nullptr, kStackBytes + page, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS, -1, 0);
            if (m == MAP_FAILED || mprotect(m, page, PROT_NONE) != 0) {
                fprintf(stderr, "vh_ref: cannot map a fiber stack\n");
                abort();
            }
            f->stack = static_cast<char*>(m) + page;
            if (getcontext(&f->ctx) != 0) abort();
            fibers.push_back(f);
        }
        return fibers[i];
    }
};

thread_local Scheduler sched;

void fiber_entry()
{
    Fiber* f = sched.current;
    sched.fn(sched.arg);
    f->state = DONE;
    /* returns to sched.main through uc_link */
}

void start(Fiber* f, uint3 tid)
{
    f->ctx.uc_stack.ss_sp = f->stack;
    f->ctx.uc_stack.ss_size = kStackBytes;
    f->ctx.uc_link = &sched.main;
    makecontext(&f->ctx, fiber_entry, 0);
    f->tid = tid;
    f->state = RUNNING;
}

void resume(Fiber* f)
{
    threadIdx = f->tid;
    f->state = RUNNING;
    sched.current = f;
    if (swapcontext(&sched.main, &f->ctx) != 0) abort();
    sched.current = nullptr;
}

}  // namespace

void vhr_barrier()
{
    Fiber* f = sched.current;
    if (!f) {
        fprintf(stderr, "vh_ref: __syncthreads reached by thread (%u, %u, %u) of block (%u, %u, %u), but not by "
                "thread (0, 0, 0)\n", threadIdx.x, threadIdx.y, threadIdx.z, blockIdx.x, blockIdx.y, blockIdx.z);
        abort();
    }
    f->state = AT_BARRIER;
    if (swapcontext(&f->ctx, &sched.main) != 0) abort();
}

void vhr_run_workgroup(vhr_thread_fn fn, void* arg, dim3 block)
{
    const size_t n = (size_t)block.x * block.y * block.z;
    if (n == 0) return;
    if (sched.current) {
        fprintf(stderr, "vh_ref: a launch from inside a kernel is not emulated\n");
        abort();
    }
    sched.fn = fn;
    sched.arg = arg;

    Fiber* first = sched.fiber(0);
    start(first, make_uint3(0, 0, 0));
    resume(first);
    if (first->state == DONE) {
        /* no barrier: the rest one after the other, without fibers */
        for (unsigned int tz = 0; tz < block.z; tz++)
        for (unsigned int ty = 0; ty < block.y; ty++)
        for (unsigned int tx = 0; tx < block.x; tx++) {
            if (tx == 0 && ty == 0 && tz == 0) continue;
            threadIdx.x = tx; threadIdx.y = ty; threadIdx.z = tz;
            fn(arg);
        }
        return;
    }

    /* the first thread waits at a barrier: every thread on a fiber */
    size_t i = 1;
    for (unsigned int tz = 0; tz < block.z; tz++)
    for (unsigned int ty = 0; ty < block.y; ty++)
    for (unsigned int tx = 0; tx < block.x; tx++) {
        if (tx == 0 && ty == 0 && tz == 0) continue;
        Fiber* f = sched.fiber(i++);
        start(f, make_uint3(tx, ty, tz));
        resume(f);
    }
    for (unsigned int round = 1;; round++) {
        size_t waiting = 0, done = 0;
        for (size_t k = 0; k < n; k++) {
            waiting += sched.fibers[k]->state == AT_BARRIER;
            done += sched.fibers[k]->state == DONE;
        }
        if (done == n) return;
        if (waiting != n) {
            fprintf(stderr, "vh_ref: block (%u, %u, %u): barrier %u reached by %zu of %zu threads; %zu returned\n",
                    blockIdx.x, blockIdx.y, blockIdx.z, round, waiting, n, done);
            abort();
        }
        for (size_t k = 0; k < n; k++) resume(sched.fibers[k]);
    }
}
