// host.h — what every handle's host half shares: the error text, HIP_TRY, the device guard,
// device blocks that grow and their release, the dynamic-LDS opt-in, the entry checks and
// env_args, the head of a kernel's argument block.
//
// A fragment of shipenv.hip's translation unit, included after se_env inside the host side's
// anonymous namespace; it uses kBlock and kMaxBlocks from above it. No device code.

thread_local std::string g_err;

int fail(int code, const std::string& msg) {
    g_err = msg;
    return code;
}

#define HIP_TRY(expr)                                                                        \
    do {                                                                                     \
        hipError_t e_ = (expr);                                                              \
        if (e_ != hipSuccess)                                                                \
            return fail(SE_EHIP, std::string(#expr) + ": " + hipGetErrorString(e_));        \
    } while (0)

struct DeviceGuard {
    int prev = -1;
    explicit DeviceGuard(int dev) {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        if (prev != dev) (void)hipSetDevice(dev);
    }
    ~DeviceGuard() {
        int cur = -1;
        if (prev >= 0 && hipGetDevice(&cur) == hipSuccess && cur != prev) (void)hipSetDevice(prev);
    }
};

int grid_for(int64_t items, int cap = kMaxBlocks) {
    int64_t b = (items + kBlock - 1) / kBlock;
    if (b < 1) b = 1;
    if (b > cap) b = cap;
    return (int)b;
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }

// ---------------------------------------------------------------- device blocks
// hipFree of every block that is not null: all are released whatever fails, and the first
// failure is returned. A destroy calls it and then always deletes its handle.
hipError_t device_free(std::initializer_list<void*> blocks) {
    hipError_t first = hipSuccess;
    for (void* p : blocks) {
        const hipError_t e = p ? hipFree(p) : hipSuccess;
        if (first == hipSuccess) first = e;
    }
    return first;
}

// At least `need` bytes behind p, whose capacity in bytes is cap. A block that suffices stays.
// Otherwise the old one goes and the owner holds (null, 0) until the new one is allocated: after
// a failed hipMalloc the next call allocates again and never passes a null pointer on.
template <typename T>
int device_reserve(T*& p, size_t& cap, size_t need) {
    if (need <= cap) return SE_OK;
    T* const old = p;
    p = nullptr;
    cap = 0;
    HIP_TRY(device_free({old}));
    HIP_TRY(hipMalloc(&p, need));
    cap = need;
    return SE_OK;
}

// ---------------------------------------------------------------- dynamic LDS
constexpr size_t kLdsDefault = 64 * 1024;  // what a launch may ask for without opting in
constexpr size_t kLdsMax = 160 * 1024;     // a workgroup's whole LDS

size_t lds_bytes(const se_env* env) { return (size_t)env->dims.padded() * 4; }

// Lets kKernel ask for up to `bytes` of dynamic LDS. hipFuncSetAttribute(MaxDynamicSharedMemorySize)
// is per device: the instantiation's flag holds a bit per device it has been set on (devices >= 64
// set it on every call), so no call is left on the launch path after the first.
template <auto kKernel>
int allow_lds(size_t bytes, int device) {
    static std::atomic<uint64_t> done{0};
    const uint64_t bit = device >= 0 && device < 64 ? 1ull << device : 0ull;
    if (bit && (done.load(std::memory_order_acquire) & bit)) return SE_OK;
    HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(kKernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                (int)bytes));
    done.fetch_or(bit, std::memory_order_acq_rel);
    return SE_OK;
}

// The dynamic LDS of a kernel that stages the world image and nothing else: lds is the image's
// size, and kKernel is opted in only where that is past what a launch gets without asking.
template <auto kKernel>
int world_lds(const se_env* env, size_t& lds) {
    lds = lds_bytes(env);
    if (lds > kLdsMax) return fail(SE_EINVAL, "the world image exceeds the LDS");
    return lds > kLdsDefault ? allow_lds<kKernel>(kLdsMax, env->device) : SE_OK;
}

// ---------------------------------------------------------------- entry checks
int check_ready(se_env* env) {
    if (!env) return fail(SE_EINVAL, "null env");
    if (!env->bound) return fail(SE_ESTATE, "se_bind has not been called");
    return SE_OK;
}

// ---------------------------------------------------------------- kernel arguments
// The head of a kernel's argument block (EnvArgs, env_core.h): an entry point assigns it once
// and then the kernel's own fields.
EnvArgs env_args(const se_env* env) {
    return EnvArgs{env->d_world, env->dims, env->n, env->env_base, env->seed, env->st};
}
