// The per-batch descriptor tables of the image stages (resize, JPEG decode, overlay + encode, heat maps) and the interval timer
// of the stages and the trainer.  Included by rn_internal.h (RN_HIP, rn_set_error and DeviceGuard come from there).
//
// A stage keeps TWO sets of its tables.  A call acquires the set that the call before the previous one used -- waiting on the host
// for that call's launches -- fills the page-locked host arrays, uploads them and launches on the handle's stream, and retires the
// set behind its launches.  So back-to-back calls on one stream never rewrite a table, host or device, that a copy or a launch
// still reads, and no property of the runtime's pageable-memory copies is relied on.
#pragma once

struct rn_owner {                      // (what follows owns what it points to and is freed with the state that holds it)
    rn_owner() = default;
    rn_owner(const rn_owner&) = delete;
    rn_owner& operator=(const rn_owner&) = delete;
};

// A typed page-locked host array and a device array of the same length.
template <typename T>
struct rn_table : rn_owner {
    T* host = nullptr;
    T* dev = nullptr;
    size_t cap = 0;                    // entries

    ~rn_table() { free(); }

    int alloc(size_t count) {
        RN_HIP(hipHostMalloc(reinterpret_cast<void**>(&host), count * sizeof(T), hipHostMallocDefault));
        RN_HIP(hipMalloc(reinterpret_cast<void**>(&dev), count * sizeof(T)));
        cap = count;
        return RN_OK;
    }
    // room for `need` entries (a quarter is added when it has to grow); the set is idle, the old contents are dropped
    int grow(size_t need) {
        if (need <= cap) return RN_OK;
        free();
        return alloc(need + need / 4);
    }
    int upload(size_t n, hipStream_t s) const {
        RN_HIP(hipMemcpyAsync(dev, host, n * sizeof(T), hipMemcpyHostToDevice, s));
        return RN_OK;
    }
    void free() {
        if (host) (void)hipHostFree(host);
        if (dev) (void)hipFree(dev);
        host = dev = nullptr;
        cap = 0;
    }
};

// Which of a stage's two sets the next call fills.  One rotation guards everything the stage keeps per set.
struct rn_rotation : rn_owner {
    hipEvent_t done[2] = {nullptr, nullptr};
    bool used[2] = {false, false};
    int next = 0;

    ~rn_rotation() {
        for (hipEvent_t e : done)
            if (e) (void)hipEventDestroy(e);
    }

    int create() {
        for (hipEvent_t& e : done) RN_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        return RN_OK;
    }
    // The idle set.  Changes nothing: a call that fails before it retires has enqueued nothing, and the next call gets the same set.
    int acquire(int* set) const {
        if (used[next]) RN_HIP(hipEventSynchronize(done[next]));
        *set = next;
        return RN_OK;
    }
    // behind the last launch that reads the acquired set
    int retire(hipStream_t s) {
        RN_HIP(hipEventRecord(done[next], s));
        used[next] = true;
        next ^= 1;
        return RN_OK;
    }
};

// Device time between two points of a stream.
struct rn_timer : rn_owner {
    hipEvent_t t0 = nullptr, t1 = nullptr;
    bool timed = false;

    ~rn_timer() {
        for (hipEvent_t e : {t0, t1})
            if (e) (void)hipEventDestroy(e);
    }

    int create() {
        RN_HIP(hipEventCreate(&t0));
        RN_HIP(hipEventCreate(&t1));
        return RN_OK;
    }
    int start(hipStream_t s) {
        timed = false;
        RN_HIP(hipEventRecord(t0, s));
        return RN_OK;
    }
    int stop(hipStream_t s) {
        RN_HIP(hipEventRecord(t1, s));
        timed = true;
        return RN_OK;
    }
    // The body of a *_last_*_ms entry point: `owner` is its handle (or trainer) and `t` the owner's timer, null while the state that
    // holds it does not exist.  Waits for the interval's end.
    static int read(const char* who, const void* owner, const rn_timer* t, const char* never_run, int device, float* ms) {
        if (!owner || !ms) {
            rn_set_error("%s: null argument", who);
            return RN_E_INVALID;
        }
        if (!t || !t->timed) {
            rn_set_error("%s: %s", who, never_run);
            return RN_E_STATE;
        }
        DeviceGuard guard(device);
        RN_HIP(hipEventSynchronize(t->t1));
        RN_HIP(hipEventElapsedTime(ms, t->t0, t->t1));
        return RN_OK;
    }
};
