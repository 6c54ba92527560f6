// One value per device ordinal, filled on first use: where a launcher keeps a "done once" fact that belongs to the DEVICE (a process
// may drive several GPUs, one host thread each: nn.DataParallel replicas).  Plain C++17, no HIP: builds with the host compiler
// alone (tests/per_device_main.cpp runs it under the thread and address sanitizers).
#pragma once
#include <atomic>
#include <mutex>
#include <optional>

#define M3D_MAX_DEVICES 64

template <typename T>
class PerDevice {
public:
    // The slot of `dev`, filled by `init()` (-> std::optional<T>) the first time it succeeds: published with a release store, read
    // with an acquire load, filled under a mutex -- every caller sees the slot's one value.  A failed init (nullopt) is handed back
    // and NOT remembered: the next call tries again.  An ordinal outside [0, M3D_MAX_DEVICES) has no slot: init runs on every call.
    template <typename Init>
    std::optional<T> get(int dev, Init &&init)
    {
        if (dev < 0 || dev >= M3D_MAX_DEVICES) return init();
        Slot &s = slots_[dev];
        if (!s.ready.load(std::memory_order_acquire)) {
            std::lock_guard<std::mutex> lock(fill_);
            if (!s.ready.load(std::memory_order_relaxed)) {
                const std::optional<T> v = init();
                if (!v) return v;
                s.value = *v;
                s.ready.store(true, std::memory_order_release);
            }
        }
        return s.value;
    }

private:
    struct Slot {
        std::atomic<bool> ready{false};
        T value{};
    };
    Slot slots_[M3D_MAX_DEVICES];
    std::mutex fill_;
};
