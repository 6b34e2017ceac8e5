// stream_gate.cpp — what a caller of the library does on its own HIP stream, for tests/test_caller_stream_gpu.py: a stream, copies
// on it ("earlier work" and "later work"), and a gate: a host function queued on the stream that holds everything queued behind
// it back for a fixed time.  The gate opens by itself; nothing here waits for anything a test has to signal.  No kernel.  Built
// by build.build_stream_gate() into libmrt_stream_gate.so, loaded by the tests alone; it links the libamdhip64 libmrt_hip.so links.
#include <atomic>
#include <chrono>
#include <new>
#include <thread>
#include <hip/hip_runtime.h>

namespace {

struct Gate {
	std::atomic<int> started{0}, done{0};
	int ms = 0;
};

void gate_body(void *user)
{
	Gate *g = static_cast<Gate *>(user);
	g->started.store(1, std::memory_order_release);
	std::this_thread::sleep_for(std::chrono::milliseconds(g->ms));
	g->done.store(1, std::memory_order_release);
}

} // namespace

extern "C" {

// A stream of device `device` that does not synchronise with the null stream.  Returns the hipError_t.
int sg_stream_create(int device, void **out)
{
	if (!out) return (int)hipErrorInvalidValue;
	*out = nullptr;
	hipError_t e = hipSetDevice(device);
	hipStream_t s = nullptr;
	if (e == hipSuccess) e = hipStreamCreateWithFlags(&s, hipStreamNonBlocking);
	if (e == hipSuccess) *out = s;
	return (int)e;
}

int sg_stream_destroy(void *stream) { return (int)hipStreamDestroy((hipStream_t)stream); }

int sg_stream_synchronize(void *stream) { return (int)hipStreamSynchronize((hipStream_t)stream); }

// Queues the gate on `stream`: work queued behind it starts after it has slept `ms` milliseconds.  *out: the handle for
// sg_gate_started / sg_gate_done, freed by sg_gate_free once done.
int sg_gate(void *stream, int ms, void **out)
{
	if (!out || ms < 0) return (int)hipErrorInvalidValue;
	Gate *g = new (std::nothrow) Gate();
	if (!g) return (int)hipErrorOutOfMemory;
	g->ms = ms;
	const hipError_t e = hipLaunchHostFunc((hipStream_t)stream, gate_body, g);
	if (e != hipSuccess) { delete g; g = nullptr; }
	*out = g;
	return (int)e;
}

int sg_gate_started(const void *gate) { return static_cast<const Gate *>(gate)->started.load(std::memory_order_acquire); }

int sg_gate_done(const void *gate) { return static_cast<const Gate *>(gate)->done.load(std::memory_order_acquire); }

// Only after the gate is done (the stream's thread still uses it before): 0, else -1 and nothing is freed.
int sg_gate_free(void *gate)
{
	Gate *g = static_cast<Gate *>(gate);
	if (!g || !g->done.load(std::memory_order_acquire)) return -1;
	delete g;
	return 0;
}

// The caller's own work: a device-to-device copy queued on `stream`.
int sg_copy(void *stream, void *dst, const void *src, size_t bytes)
{
	return (int)hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, (hipStream_t)stream);
}

} // extern "C"
