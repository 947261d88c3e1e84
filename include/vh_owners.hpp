// vh_owners.hpp -- vh::Error, and who owns device memory, pinned host memory, events and streams: std::unique_ptr with
// deleters that are declared here and defined in the library (voxelhashing_amd/csrc/vh_host.cpp).  A class that holds
// its resources through these types frees nothing by hand; C++ gives the order: the destructor's body first, then the
// members in reverse order of declaration -- also for an object whose constructor throws half-way, for the members
// made so far.  Needs no HIP headers.
#ifndef VH_OWNERS_HPP
#define VH_OWNERS_HPP

#include <cstddef>
#include <memory>
#include <stdexcept>
#include <string>
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

} // namespace vh

#endif // VH_OWNERS_HPP
