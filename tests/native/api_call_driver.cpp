// api_call_driver.cpp — stand-alone check of the entry wrapper of the C-ABI (csrc/opd_device.h: api_call; csrc/opd_host.h:
// api_call_unlocked) on the CPU: what a throwing body returns and reports, nesting on one thread, a capture's exclusive hold inside an
// entry point against a second thread's entry, and the lock-free form against an exclusive holder.  Makes no HIP call.  Linked with
// csrc/opd_host.cpp (the lock, the error text, opd_last_error, opd_person_nms); tests/test_api_call_cpu.py builds and runs it.
#include <stdio.h>
#include <string.h>

#include <atomic>
#include <chrono>
#include <future>
#include <thread>

#include "opd_device.h"

using namespace opd;

static std::atomic<int> failures{0};
#define EXPECT(cond)                                                        \
    do {                                                                    \
        if (!(cond)) { ++failures; printf("FAILED line %d: %s\n", __LINE__, #cond); } \
    } while (0)

static bool lock_is_free() {   // nobody holds the entry-point lock, shared or exclusive
    if (!g_api_mu.try_lock()) return false;
    g_api_mu.unlock();
    return true;
}
static bool names(const char* entry) { return strstr(opd_last_error(), entry) != nullptr; }

template <typename Call>
static void throwing_bodies(const char* form, Call&& call) {
    EXPECT(call("entry_bad_alloc", []() -> int { throw std::bad_alloc(); }, false) == OPD_ENOMEM);
    EXPECT(names("entry_bad_alloc") && names("out of host memory"));
    EXPECT(call("entry_runtime_error", []() -> int { throw std::runtime_error("boom"); }, false) == OPD_EINVAL);
    EXPECT(names("entry_runtime_error") && names("boom"));
    EXPECT(call("entry_out_of_range", []() -> int { throw std::out_of_range("no such key"); }, false) == OPD_EINVAL);
    EXPECT(names("entry_out_of_range") && names("no such key") && !names("weight file"));
    EXPECT(call("entry_create", []() -> int { throw std::out_of_range("model.w"); }, API_CREATE) == OPD_ESCHEMA);
    EXPECT(names("entry_create") && names("weight file lacks a tensor the model needs (model.w)"));
    EXPECT(call("entry_create_alloc", []() -> int { throw std::bad_alloc(); }, API_CREATE) == OPD_ENOMEM);   // the flavour changes out_of_range alone
    EXPECT(call("entry_int", []() -> int { throw 42; }, false) == OPD_EINVAL);
    EXPECT(names("entry_int") && names("unknown C++ exception"));
    EXPECT(call("entry_fine", []() -> int { return 7; }, false) == 7);
    EXPECT(tl_api_lock == nullptr && lock_is_free());   // every way out gave the hold back
    printf("%s: throwing bodies done\n", form);
}

int main() {
    throwing_bodies("api_call", [](const char* n, auto body, bool create) { return api_call(n, body, create); });
    throwing_bodies("api_call_unlocked", [](const char* n, auto body, bool create) { return api_call_unlocked(n, body, create); });

    // entry points call each other: the inner one takes no second hold, and its exception stays inside it
    int rc = api_call("outer", [&]() -> int {
        std::shared_lock<std::shared_mutex>* mine = tl_api_lock;
        EXPECT(mine && mine->owns_lock());
        const int inner = api_call("inner", [&]() -> int {
            EXPECT(tl_api_lock == mine);
            return api_call("innermost", []() -> int { throw std::runtime_error("deep"); });
        });
        EXPECT(inner == OPD_EINVAL && names("innermost"));
        EXPECT(tl_api_lock == mine && mine->owns_lock());   // the outer hold survives the inner calls
        return 11;
    });
    EXPECT(rc == 11 && tl_api_lock == nullptr && lock_is_free());
    printf("nesting done\n");

    // a capture inside an entry point: the thread's shared hold is handed back, the lock taken exclusively; a second thread's entry waits
    // for the capture's end and then proceeds beside the first, whose shared hold is back
    std::atomic<int> second{0};   // 1: about to enter, 2: inside its body
    std::thread other;
    rc = api_call("capturing", [&]() -> int {
        std::shared_lock<std::shared_mutex>* mine = tl_api_lock;
        {
            CaptureExclusive alone;
            EXPECT(!mine->owns_lock());
            other = std::thread([&] {
                EXPECT(!g_api_mu.try_lock_shared());   // (exclusively held: an entry would wait)
                second = 1;
                EXPECT(api_call("second", [&]() -> int { second = 2; return 5; }) == 5);
            });
            while (second.load() == 0) std::this_thread::yield();
            std::this_thread::sleep_for(std::chrono::milliseconds(20));   // (time for a wrapper that did not wait to show it)
            EXPECT(second.load() == 1);
        }
        EXPECT(mine->owns_lock());
        other.join();   // proceeds while this thread holds the lock shared again
        EXPECT(second.load() == 2);
        return 3;
    });
    EXPECT(rc == 3 && tl_api_lock == nullptr && lock_is_free());
    printf("capture done\n");

    // the lock-free form, and the real lock-free entries of opd_host.cpp, do not wait behind an exclusive holder
    g_api_mu.lock();
    auto free_call = std::async(std::launch::async, [] {
        int ok = api_call_unlocked("lock_free", []() -> int { return 9; }) == 9;
        ok += opd_person_nms(nullptr, -1, 0, 0.5f) == OPD_EINVAL && strstr(opd_last_error(), "opd_person_nms: bad arguments") != nullptr;
        return ok;
    });
    const bool came_back = free_call.wait_for(std::chrono::seconds(20)) == std::future_status::ready;
    g_api_mu.unlock();
    EXPECT(came_back);
    EXPECT(free_call.get() == 2);
    EXPECT(lock_is_free());
    printf("lock-free done\n");

    printf("api_call cases done, failures %d\n", failures.load());
    return failures.load() ? 1 : 0;
}
