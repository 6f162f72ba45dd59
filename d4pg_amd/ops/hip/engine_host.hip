// Host support for the Engine class: plain C++, no device code.  Included by
// engine.hip after the device parts (a fragment, not a stand-alone source).
//
//   launch()      every kernel launch, with its status checked
//   DevicePool    one device allocation, carved twice by one function
//   GraphSlot     one captured hipGraph and its executable
//   Stream/Event  owning handles
//
// A new pool, graph, stream or event of the engine is a member of one of
// these types, never a raw handle with a hand-written release.

#include <string>
#include <utility>

namespace d4pg {

template <class T> struct AsIs { using type = T; };

// kernel<<<grid, block, lds_bytes, stream>>>(args...), checked.  Each
// argument converts to the kernel's parameter type as in the call syntax
// (the parameter pack is deduced from the kernel alone), and is passed by
// address: a StepArgs is not copied on the way.  The status is the launch
// call's own return value, never the thread's last-error word, which torch
// and RCCL share.  Valid inside stream capture.
template <class... P>
void launch(void (*kernel)(P...), dim3 grid, dim3 block, size_t lds_bytes,
            hipStream_t stream, const typename AsIs<P>::type&... args) {
    void* argv[] = {const_cast<void*>(static_cast<const void*>(&args))...,
                    nullptr};
    hipError_t e = hipLaunchKernel(reinterpret_cast<const void*>(kernel),
                                   grid, block, argv, lds_bytes, stream);
    if (e == hipSuccess) return;
    const char* name = hipKernelNameRefByPtr(
        reinterpret_cast<const void*>(kernel), stream);
    throw std::runtime_error(
        std::string("HIP error ") + hipGetErrorString(e) + " launching " +
        (name ? name : "a kernel") + " (grid " + std::to_string(grid.x) +
        ", block " + std::to_string(block.x) + ", lds " +
        std::to_string(lds_bytes) + " bytes)");
}

// One device allocation.  build(carve) runs carve(pool) twice, first with a
// null base to size the pool, then to point the buffers into the cleared
// allocation, so sizes and pointers cannot drift apart.  carve names each
// buffer once, as pool.take(pointer, nelem).
class DevicePool {
    char* base_ = nullptr;
    long off_ = 0;

public:
    DevicePool() = default;
    DevicePool(DevicePool&& o) noexcept
        : base_(std::exchange(o.base_, nullptr)), off_(o.off_) {}
    DevicePool& operator=(DevicePool&& o) noexcept {
        if (this != &o) {
            reset();
            base_ = std::exchange(o.base_, nullptr);
            off_ = o.off_;
        }
        return *this;
    }
    ~DevicePool() { reset(); }

    explicit operator bool() const { return base_ != nullptr; }

    // nelem elements of *p, rounded up to 256 bytes; null in the count pass.
    // A zero-length entry takes no room and shares the next one's address.
    template <class T>
    void take(T*& p, long nelem) {
        p = base_ ? reinterpret_cast<T*>(base_ + off_) : nullptr;
        off_ += (nelem * (long)sizeof(T) + 255) & ~255L;
    }

    template <class Carve>
    void build(Carve&& carve) {
        reset();
        off_ = 0;
        carve(*this);                           // count pass (null base)
        const long total = off_;
        void* p = nullptr;
        HIP_CHECK(hipMalloc(&p, total));
        base_ = static_cast<char*>(p);
        try {
            HIP_CHECK(hipMemset(base_, 0, total));
            off_ = 0;
            carve(*this);                       // assign pass
            // the clear went to the null stream; the engine's streams are
            // non-blocking
            HIP_CHECK(hipDeviceSynchronize());
        } catch (...) {
            reset();
            throw;
        }
    }

    void reset() {
        if (base_) (void)hipFree(base_);
        base_ = nullptr;
    }
};

// One captured graph and its executable.
class GraphSlot {
    hipGraph_t graph_ = nullptr;
    hipGraphExec_t exec_ = nullptr;

public:
    GraphSlot() = default;
    GraphSlot(const GraphSlot&) = delete;
    GraphSlot& operator=(const GraphSlot&) = delete;
    ~GraphSlot() { reset(); }

    explicit operator bool() const { return exec_ != nullptr; }

    // Capture enqueue() on `stream` and instantiate it, on first use only.
    // Whatever fails in between, the capture is ended, the slot is left
    // empty and the stream out of capture mode before the error goes on.
    template <class Enqueue>
    void ensure(hipStream_t stream, Enqueue&& enqueue) {
        if (exec_) return;
        HIP_CHECK(hipStreamBeginCapture(stream,
                                        hipStreamCaptureModeThreadLocal));
        try {
            enqueue();
            HIP_CHECK(hipStreamEndCapture(stream, &graph_));
            HIP_CHECK(hipGraphInstantiate(&exec_, graph_, nullptr, nullptr,
                                          0));
        } catch (...) {
            // enqueue threw: the capture is still open
            hipStreamCaptureStatus s = hipStreamCaptureStatusNone;
            if (hipStreamIsCapturing(stream, &s) == hipSuccess &&
                s != hipStreamCaptureStatusNone)
                (void)hipStreamEndCapture(stream, &graph_);
            reset();
            throw;
        }
    }

    void launch(hipStream_t stream) {
        HIP_CHECK(hipGraphLaunch(exec_, stream));
    }

    void reset() {
        if (exec_) (void)hipGraphExecDestroy(exec_);
        if (graph_) (void)hipGraphDestroy(graph_);
        exec_ = nullptr;
        graph_ = nullptr;
    }
};

// An owned stream or event: converts to its handle, destroyed with the owner.
template <class H, hipError_t (*Destroy)(H)>
class Owned {
    H h_ = nullptr;

public:
    Owned() = default;
    Owned(Owned&& o) noexcept : h_(std::exchange(o.h_, nullptr)) {}
    Owned& operator=(Owned&& o) noexcept {
        if (this != &o) { reset(); h_ = std::exchange(o.h_, nullptr); }
        return *this;
    }
    ~Owned() { reset(); }

    operator H() const { return h_; }
    H* put() { reset(); return &h_; }       // for the create call

    void reset() {
        if (h_) (void)Destroy(h_);
        h_ = nullptr;
    }
};
using Stream = Owned<hipStream_t, hipStreamDestroy>;
using Event = Owned<hipEvent_t, hipEventDestroy>;

}  // namespace d4pg
