"""What the host reads of the words the device publishes (include/vh_owners.hpp: loadRelaxed, loadAcquire, nextTag,
spinUntil, arrived, waitArrived, vh::Published), without a device: a stand-alone C++ program in which a std::thread plays
the device -- body words stored relaxed, then the tag with release -- into ordinary memory.  The same source is built a
second time with ThreadSanitizer and run directly."""
import os
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROGRAM = r"""
#include "vh_owners.hpp"
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <thread>
// the library's allocators, in ordinary memory (the program does not link the library): filled with ones, so that
// Published has to zero its record itself; the "device alias" is the host pointer
void* vh::pinnedAllocBytes(size_t bytes, bool, const char*) { void* p = std::malloc(bytes); std::memset(p, 0xff, bytes); return p; }
void* vh::deviceAlias(void* host, const char*) { return host; }
void vh::PinnedFree::operator()(void* p) const noexcept { std::free(p); }
#define EXPECT(cond) do { if (!(cond)) { std::printf("line %d: %s\n", __LINE__, #cond); return 1; } } while (0)

enum { kWords = 12, kTagWord = vh::Published::kTagWord };
static uint32_t bodyWord(uint32_t tag, uint32_t i) { return tag * 2654435761u + i * 40503u + 1u; }
// publish_tag's order: the body, then the tag with release
static void publish(uint32_t* record, uint32_t tag)
{
    for (uint32_t i = 0; i < kWords; i++)
        if (i != kTagWord) __atomic_store_n(&record[i], bodyWord(tag, i), __ATOMIC_RELAXED);
    __atomic_store_n(&record[kTagWord], tag, __ATOMIC_RELEASE);
}
static double secondsSince(std::chrono::steady_clock::time_point t0)
{
    return std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
}

// a device that publishes into `record` every tag handed to it through `launch` (0: quit)
struct Device {
    uint32_t* record;
    std::atomic<uint32_t> launch{ 0 };
    std::atomic<bool> quit{ false };
    std::thread thread;
    explicit Device(uint32_t* r) : record(r), thread([this] { run(); }) {}
    ~Device() { quit.store(true); thread.join(); }
    void run()
    {
        uint32_t last = 0;
        for (;;) {
            uint32_t tag;
            while ((tag = launch.load(std::memory_order_acquire)) == last) {
                if (quit.load()) return;
                std::this_thread::yield();
            }
            publish(record, tag);
            last = tag;
        }
    }
};

static int rounds()
{
    const int kRounds = 4000;
    // through the owner: tags from 1
    {
        vh::Published rec(kWords, "record");
        for (uint32_t i = 0; i < kWords; i++) EXPECT(vh::loadRelaxed(rec.device() + i) == 0u); // zeroed at creation
        Device dev(rec.device());
        for (int r = 0; r < kRounds; r++) {
            const uint32_t tag = rec.nextTag();
            EXPECT(tag == (uint32_t)r + 1u);
            dev.launch.store(tag, std::memory_order_release);
            const vh::Waited w = rec.wait(20.0, (r & 1) != 0);
            EXPECT(w.ok && w.seconds >= 0.0 && w.seconds < 20.0);
            EXPECT(rec.arrived());
            for (uint32_t i = 0; i < kWords; i++)
                if (i != kTagWord) EXPECT(rec.word(i) == bodyWord(tag, i));
        }
    }
    // the free functions on a plain array, across the wrap of the tag
    {
        uint32_t record[kWords] = { 0 };
        Device dev(record);
        uint32_t tag = 0xffffffffu - (uint32_t)kRounds / 2u;
        bool wrapped = false;
        for (int r = 0; r < kRounds; r++) {
            const uint32_t before = tag, t = vh::nextTag(tag);
            EXPECT(t == tag && t != 0u && t != before);
            if (before == 0xffffffffu) { EXPECT(t == 1u); wrapped = true; }
            dev.launch.store(t, std::memory_order_release);
            const vh::Waited w = vh::waitArrived(&record[kTagWord], t, 20.0, (r & 1) != 0);
            EXPECT(w.ok);
            for (uint32_t i = 0; i < kWords; i++)
                if (i != kTagWord) EXPECT(vh::loadRelaxed(&record[i]) == bodyWord(t, i));
        }
        EXPECT(wrapped);
    }
    return 0;
}

static int nextTagSkipsZero()
{
    uint32_t t = 0;
    EXPECT(vh::nextTag(t) == 1u && t == 1u);
    t = 0xfffffffeu;
    EXPECT(vh::nextTag(t) == 0xffffffffu);
    EXPECT(vh::nextTag(t) == 1u && t == 1u); // 0 is the tag of a record nothing was published to
    EXPECT(vh::nextTag(t) == 2u);
    return 0;
}

static int timeOut()
{
    const double limit = 0.05;
    for (int yield = 0; yield < 2; yield++) {
        uint32_t record[kWords] = { 0 };
        const auto t0 = std::chrono::steady_clock::now();
        const vh::Waited w = vh::waitArrived(&record[kTagWord], 7u, limit, yield != 0);
        const double took = secondsSince(t0);
        EXPECT(!w.ok);
        EXPECT(w.seconds >= limit && took >= limit && w.seconds <= took);
    }
    vh::Published rec(4, "record");
    (void)rec.nextTag();
    const auto t0 = std::chrono::steady_clock::now();
    EXPECT(!rec.wait(limit).ok && secondsSince(t0) >= limit);
    // a condition that holds at the first look costs no time and no clock
    const vh::Waited w = vh::spinUntil([] { return true; }, limit, false);
    EXPECT(w.ok && w.seconds == 0.0);
    return 0;
}

static int look()
{
    vh::Published rec(kWords, "record");
    const uint32_t tag = rec.nextTag();
    EXPECT(!rec.arrived() && !vh::arrived(rec.device() + kTagWord, tag));
    std::thread device([&] { publish(rec.device(), tag); });
    device.join();
    EXPECT(rec.arrived() && vh::arrived(rec.device() + kTagWord, tag));
    EXPECT(rec.word(0) == bodyWord(tag, 0) && rec.word(kWords - 1) == bodyWord(tag, kWords - 1));
    (void)rec.nextTag();
    EXPECT(!rec.arrived()); // the record still holds the tag before
    return 0;
}

static int bothVariantsSeeTheStore()
{
    for (int yield = 0; yield < 2; yield++) {
        vh::Published rec(kWords, "record");
        const uint32_t tag = rec.nextTag();
        std::thread device([&] {
            std::this_thread::sleep_for(std::chrono::milliseconds(2));
            publish(rec.device(), tag);
        });
        const vh::Waited w = rec.wait(20.0, yield != 0);
        device.join();
        EXPECT(w.ok && w.seconds > 0.0 && w.seconds < 20.0);
        EXPECT(rec.word(1) == bodyWord(tag, 1));
    }
    return 0;
}

int main()
{
    if (nextTagSkipsZero() || look() || timeOut() || bothVariantsSeeTheStore() || rounds()) return 1;
    std::printf("ok\n");
    return 0;
}
"""


def _compile(d, name, extra):
    """object first, then the link on its own: only a link that fails may excuse the sanitizer's leg"""
    src, obj, exe = os.path.join(d, "t.cpp"), os.path.join(d, name + ".o"), os.path.join(d, name)
    if not os.path.exists(src):
        open(src, "w").write(PROGRAM)
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-pthread", "-I", os.path.join(ROOT, "include")] + extra + ["-c", src, "-o", obj])
    link = subprocess.run(["g++", "-pthread"] + extra + [obj, "-o", exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    return exe, link


def test_published_records_and_bounded_waits():
    """the body read after arrived() is the body written, over 2 x 4000 rounds with changing tags (through vh::Published
    and through the free functions on a plain array, across the tag's wrap); nextTag() skips 0; a wait for a tag that
    never comes returns "not arrived" no sooner than its limit; the look without waiting says "not yet" before the store
    and "arrived" after; the yielding and the spinning wait both see the store"""
    with tempfile.TemporaryDirectory() as d:
        exe, link = _compile(d, "t", ["-O2"])
        assert link.returncode == 0, link.stdout.decode()
        res = subprocess.run([exe], stdout=subprocess.PIPE, timeout=240)
        assert res.returncode == 0 and res.stdout.decode().strip() == "ok", res.stdout.decode()


def test_published_records_under_thread_sanitizer():
    """the same program under ThreadSanitizer, run directly: it reports nothing"""
    with tempfile.TemporaryDirectory() as d:
        exe, link = _compile(d, "t_tsan", ["-O1", "-g", "-fsanitize=thread"])
        if link.returncode != 0:
            pytest.skip("no ThreadSanitizer runtime to link against: " + link.stdout.decode()[-300:])
        env = dict(os.environ, TSAN_OPTIONS="halt_on_error=1 exitcode=66")
        res = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env, timeout=480)
        assert res.returncode == 0 and res.stdout.decode().strip() == "ok" and b"ThreadSanitizer" not in res.stderr, \
            res.stdout.decode() + res.stderr.decode()[-3000:]
