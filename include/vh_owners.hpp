// vh_owners.hpp -- vh::Error, and who owns device memory, pinned host memory, events and streams: std::unique_ptr with
// deleters that are declared here and defined in the library (voxelhashing_amd/csrc/vh_host.cpp).  A class that holds
// its resources through these types frees nothing by hand; C++ gives the order: the destructor's body first, then the
// members in reverse order of declaration -- also for an object whose constructor throws half-way, for the members
// made so far.  Below them: how the host reads what the device publishes into mapped memory.  Needs no HIP headers.
#ifndef VH_OWNERS_HPP
#define VH_OWNERS_HPP

#include <chrono>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <memory>
#include <stdexcept>
#include <string>
#include <thread>
#include <utility>

namespace vh {

struct Error : public std::runtime_error {
    int code;
    Error(int c, const std::string& what) : std::runtime_error(what), code(c) {}
};

struct DeviceFree { void operator()(void* p) const noexcept; };    // hipFree
struct PinnedFree { void operator()(void* p) const noexcept; };    // hipHostFree
struct EventDestroy { void operator()(void* e) const noexcept; };  // hipEventDestroy
struct StreamDestroy { void operator()(void* s) const noexcept; }; // hipStreamDestroy

template <class T> using DevicePtr = std::unique_ptr<T[], DeviceFree>;
template <class T> using PinnedPtr = std::unique_ptr<T[], PinnedFree>;
typedef std::unique_ptr<void, EventDestroy> Event;   // a hipEvent_t
typedef std::unique_ptr<void, StreamDestroy> Stream; // a hipStream_t

// these throw vh::Error(-hipError_t, what + ": " + the runtime's text)
void* deviceAllocBytes(size_t bytes, const char* what);
void* pinnedAllocBytes(size_t bytes, bool mapped, const char* what);
void* deviceAlias(void* mappedHost, const char* what); // hipHostGetDevicePointer
// device-scope release where the runtime has it: these events order streams of one device or time them, nothing on the
// host reads memory behind them (a default event record makes the queue write back its caches: ~6 us of idle queue)
Event makeEvent(bool timing);
Stream makeStream(const char* what); // non-blocking

// n elements, at least one
template <class T> DevicePtr<T> deviceAlloc(size_t n, const char* what)
{
    return DevicePtr<T>(static_cast<T*>(deviceAllocBytes(sizeof(T) * (n ? n : 1), what)));
}
template <class T> PinnedPtr<T> pinnedAlloc(size_t n, const char* what)
{
    return PinnedPtr<T>(static_cast<T*>(pinnedAllocBytes(sizeof(T) * (n ? n : 1), false, what)));
}

// mapped pinned host memory and its device alias: what the device publishes to the host without a copy
template <class T> class Mapped {
public:
    Mapped() = default;
    Mapped(size_t n, const char* what)
        : m_host(static_cast<T*>(pinnedAllocBytes(sizeof(T) * (n ? n : 1), true, what))), m_device(static_cast<T*>(deviceAlias(m_host.get(), what))) {}
    Mapped(Mapped&& o) noexcept : m_host(std::move(o.m_host)), m_device(std::exchange(o.m_device, nullptr)) {}
    Mapped& operator=(Mapped&& o) noexcept
    {
        m_host = std::move(o.m_host);
        m_device = std::exchange(o.m_device, nullptr);
        return *this;
    }
    T* host() const { return m_host.get(); }
    T* device() const { return m_device; }

private:
    PinnedPtr<T> m_host;
    T* m_device = nullptr;
};

// ---- what the device tells the host ------------------------------------------------------------------------------
// The contract both sides keep.  The device stores a record's body into mapped host memory, then the record's tag with
// release at system scope: publish_tag (vh_streaming.hip) and icp_publish (vh_icp.hip) are the writers.  The host loads
// the tag with acquire and only then the body; a tag is compared for equality with the one the host handed to the
// launch, and 0 is the tag of a record nothing has been published to.  Words the device mirrors without a tag
// ({block count, frame number}, the ray caster's longest list) are single relaxed loads: each is a value of its own
// that nothing else is read behind.  The functions take plain pointers: mapped memory is ordinary memory to the host.
// How long the host waits is said once, below; what a time-out means is each caller's.
inline uint32_t loadRelaxed(const uint32_t* word) { return __atomic_load_n(word, __ATOMIC_RELAXED); }
inline uint32_t loadAcquire(const uint32_t* word) { return __atomic_load_n(word, __ATOMIC_ACQUIRE); }
inline uint32_t nextTag(uint32_t& tag) { return ++tag ? tag : ++tag; } // never 0
const double kPublishSyncSeconds = 2.0;       // a tag of the scene's stream: then synchronise the stream and look again
const double kDeviceSilentSeconds = 30.0;     // a tag or a counter the device should long have written: then VH_ERR_TIMEOUT
const double kWorkerSilentSeconds = 40.0;     // a worker thread that may itself wait kDeviceSilentSeconds: then VH_ERR_TIMEOUT
const double kSpinBeforeSleepSeconds = 300e-6; // a thread that expects work within a frame or two: then the condition variable

// The one bounded wait: looks at pred() until it is true or limitSeconds have passed; between looks it does nothing, or
// gives the processor away if `yield`.  The steady clock is read when the first look fails and then every 256th look.
struct Waited { bool ok; double seconds; }; // seconds: how long the wait took (0 if the first look succeeded)
template <class Pred> Waited spinUntil(Pred pred, double limitSeconds, bool yield)
{
    if (pred()) return { true, 0.0 };
    const auto t0 = std::chrono::steady_clock::now();
    auto elapsed = [t0] { return std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count(); };
    for (unsigned int looks = 1;; looks++) {
        if (yield) std::this_thread::yield();
        if (pred()) return { true, elapsed() };
        if ((looks & 0xffu) == 0u && elapsed() > limitSeconds) return { false, elapsed() };
    }
}

// has `tag` been published at *tagWord?  After true the record's body may be read (loadRelaxed, or plain loads)
inline bool arrived(const uint32_t* tagWord, uint32_t tag) { return loadAcquire(tagWord) == tag; }
inline Waited waitArrived(const uint32_t* tagWord, uint32_t tag, double limitSeconds, bool yield)
{
    return spinUntil([=] { return arrived(tagWord, tag); }, limitSeconds, yield);
}

// a record of 32-bit words the way publish_tag writes it, {word 0, word 1, tag, word 3 ...}, and the tag the host expects in it
class Published {
public:
    enum { kTagWord = 2 };
    Published() = default;
    Published(size_t words, const char* what) : m_words(words, what) { std::memset(m_words.host(), 0, sizeof(uint32_t) * words); }
    uint32_t nextTag() { return vh::nextTag(m_tag); } // for the launch that will publish; never 0
    uint32_t* device() const { return m_words.device(); }
    bool arrived() const { return vh::arrived(m_words.host() + kTagWord, m_tag); }
    uint32_t word(size_t i) const { return loadRelaxed(m_words.host() + i); } // only after arrived()
    Waited wait(double limitSeconds, bool yield = false) const { return waitArrived(m_words.host() + kTagWord, m_tag, limitSeconds, yield); }

private:
    Mapped<uint32_t> m_words;
    uint32_t m_tag = 0;
};

} // namespace vh

#endif // VH_OWNERS_HPP
