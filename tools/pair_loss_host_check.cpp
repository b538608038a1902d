// Host-only driver of the argument checks of hpl_pair_grad, for a sanitizer build: no device is needed,
// every call returns before a launch (a refusal).  Build and run from the repository root:
//
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//       tools/pair_loss_host_check.cpp hplflownet_amd/csrc/pair_loss.hip -o /tmp/pair_loss_host_check && /tmp/pair_loss_host_check
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "../include/hpl_bcl.h"

namespace hpl {
static char g_err[512];
void set_error(const char *fmt, ...) {       // (index_ops.hip has the library's; this program links pair_loss.hip alone)
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof g_err, fmt, ap);
    va_end(ap);
}
}  // namespace hpl

static int failures = 0;

static void expect(bool ok, const char *what) {
    if (!ok) {
        ++failures;
        printf("FAILED: %s (last error: %s)\n", what, hpl::g_err);
    }
}

struct Grad {
    uintptr_t dflow = 0x10000, pair_loss = 0x20000, grad = 0x30000, loss = 0x40000;
    int64_t rows = 100;
    int batch = 2, loss_stride = 4;
    int run() const {
        return hpl_pair_grad((const float *)dflow, rows, batch, (const float *)pair_loss, loss_stride, (float *)grad, (float *)loss,
                             nullptr);
    }
};

int main() {
    const int64_t big = (((int64_t)1 << 31) + 2) / 3;
    auto refuse = [](int rc, const char *name, const char *what) {
        expect(rc == HPL_EINVAL && strncmp(hpl::g_err, name, strlen(name)) == 0, what);
        hpl::g_err[0] = 0;
    };
#define GRAD(what, ...) { Grad c; __VA_ARGS__; refuse(c.run(), "hpl_pair_grad", "grad: " what); }
    GRAD("batch 0", c.batch = 0)
    GRAD("batch 65", c.batch = 65)
    GRAD("nothing asked for", c.grad = c.loss = 0)
    GRAD("null dflow", c.dflow = 0)
    GRAD("loss without pair_loss", c.pair_loss = 0)
    GRAD("loss stride 0", c.loss_stride = 0)
    GRAD("negative rows", c.rows = -1)
    GRAD("rows = 2^31 / 3", c.rows = big)
    GRAD("rows = 2^60", c.rows = (int64_t)1 << 60)
    GRAD("misaligned dflow", c.dflow += 2)
    GRAD("misaligned grad", c.grad += 1)
    GRAD("misaligned pair_loss", c.pair_loss += 3)
    GRAD("misaligned loss", c.loss += 2)
    // nothing to launch: accepted without a device
    { Grad c; c.rows = 0; c.loss = 0; expect(c.run() == HPL_OK, "grad: no rows, no loss"); }
    { Grad c; c.rows = 0; c.loss = 0; c.pair_loss = 0; c.dflow += 4; c.grad += 8; expect(c.run() == HPL_OK, "grad: no rows, no pair_loss"); }
    printf(failures ? "%d check(s) failed\n" : "all checks passed\n", failures);
    return failures ? 1 : 0;
}
