// device_owners_check.hip — the owners of csrc/lscqp_device.hpp where every allocation fails: a machine without a HIP device.
// A stand-alone host program (its own main, its own lscqp_set_error_; it links nothing of the library), meant to be built with the host
// sanitizers and run where there is no GPU:
//   mkdir -p tools/_dbg
//   hipcc --offload-arch=gfx950 -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined tools/device_owners_check.hip -o tools/_dbg/device_owners_check
//   tools/_dbg/device_owners_check
// It checks that a failed allocation leaves its owner empty, that the error is LSCQP_ERR_HIP with the caller's text in front of the
// runtime's, and that moving, resetting and destroying empty owners does nothing.  On a machine WITH a device the allocations succeed and
// the program says so and checks the owners' moves on live memory instead.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <string.h>

#include <string>
#include <utility>
#include <vector>

#include "../lsc_dr_planner_amd/csrc/lscqp_device.hpp"

static int g_code = LSCQP_OK;
static std::string g_text;
extern "C" int lscqp_set_error_(int code, const char* msg) {
    g_code = code;
    g_text = msg ? msg : "";
    return code;
}

static int g_failed = 0;
#define CHECK(cond)                                                    \
    do {                                                               \
        if (!(cond)) {                                                 \
            printf("FAILED line %d: %s\n", __LINE__, #cond);           \
            g_failed++;                                                \
        }                                                              \
    } while (0)

struct Bundle {  // an option's state as the plan keeps it: owners and plain data side by side
    int n = 0;
    std::vector<int> host;
    lscqp::dev_ptr<double> a;
    lscqp::dev_ptr<int32_t> b;
};

int main() {
    int ndev = 0;
    const bool has_device = hipGetDeviceCount(&ndev) == hipSuccess && ndev > 0;
    printf("devices: %d\n", has_device ? ndev : 0);

    lscqp::dev_ptr<double> a;
    const int rc = lscqp::dev_alloc(a, 1000, "the caller's text");
    if (!has_device) {
        CHECK(rc == LSCQP_ERR_HIP && g_code == LSCQP_ERR_HIP);
        CHECK(!a);
        CHECK(g_text.rfind("the caller's text: ", 0) == 0 && g_text.size() > strlen("the caller's text: "));
        printf("error text: %s\n", g_text.c_str());
        // a zeroed allocation fails in the allocation, with the same text; an owner that held nothing still holds nothing
        lscqp::dev_ptr<int32_t> z;
        g_text.clear();
        CHECK(lscqp::dev_alloc(z, 7, "zeroed", true) == LSCQP_ERR_HIP && !z && g_text.rfind("zeroed: ", 0) == 0);
    } else {
        CHECK(rc == LSCQP_OK && a);
    }
    // hip_fail by itself
    CHECK(lscqp::hip_fail(hipErrorInvalidValue, "what") == LSCQP_ERR_HIP);
    CHECK(g_text == std::string("what: ") + hipGetErrorString(hipErrorInvalidValue));

    // moving and resetting: empty owners where nothing could be allocated, live ones otherwise
    lscqp::dev_ptr<double> b = std::move(a);
    CHECK(!a);
    a = std::move(b);
    CHECK(!b);
    b.reset();
    a.reset();
    CHECK(!a && !b);
    lscqp::pinned_ptr<int32_t> w, w2;
    w2 = std::move(w);
    w2.reset();
    CHECK(!w && !w2);

    // build-then-move of a whole state, as the setters do it
    Bundle cur, next;
    next.n = 3, next.host = {1, 2, 3};
    const int rc_a = lscqp::dev_alloc(next.a, 3, "bundle");
    CHECK(has_device ? rc_a == LSCQP_OK : (rc_a == LSCQP_ERR_HIP && !next.a));
    cur = std::move(next);
    CHECK(cur.n == 3 && cur.host.size() == 3 && !next.a && !next.b);
    cur = Bundle();  // (how a setter clears its option)
    CHECK(cur.n == 0 && cur.host.empty() && !cur.a && !cur.b);

    // the guard on a machine without a device: nothing to restore, nothing crashes
    {
        lscqp::OnDevice on(0);
        CHECK(has_device || on.prev == -1);
    }
    printf(g_failed ? "device_owners_check: %d FAILED\n" : "device_owners_check: ok\n", g_failed);
    return g_failed ? 1 : 0;
}
