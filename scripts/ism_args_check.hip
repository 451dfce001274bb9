// ism_args_check.hip -- the argument checks of iris_ism_rir (csrc/host_ops.h) as a stand-alone host program, for a run under
// the host sanitizers.  It never touches a device: refused tables return before any HIP call, and accepted ones are passed to
// the static check function, not to the launch.  Build and run (from the repository root):
//     hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -Wno-unused-function -Xarch_host -fsanitize=address,undefined \
//         -o ism_args_check scripts/ism_args_check.hip && ./ism_args_check
#include "../challenge_amd/csrc/iris_frontend.hip"

static iris_ism_src good() {
    iris_ism_src r;
    memset(&r, 0, sizeof r);
    r.dst = reinterpret_cast<float*>(8);
    r.room[0] = 3.1, r.room[1] = 4.3, r.room[2] = 2.6;
    r.src[0] = 2.05, r.src[1] = 3.12, r.src[2] = 1.57;
    r.beta = 0.5, r.n_taps = 64;
    const double mic[2][3] = {{1.13, 1.71, 1.22}, {1.23, 1.74, 1.19}};
    memcpy(r.mic, mic, sizeof mic);
    return r;
}

static int failures = 0;
static void expect(int rc, int want, const char* what) {
    if (rc != want) printf("FAIL %s: rc = %d, expected %d (%s)\n", what, rc, want, iris_last_error()), ++failures;
}

int main() {
    void* dev = reinterpret_cast<void*>(8);
    std::vector<iris_ism_src> t(3, good());
    expect(ism_check(t.data(), dev, 3, 2, 4096, 16000.0), IRIS_OK, "three good records");
    expect(ism_check(t.data(), dev, 3, IRIS_ISM_MAX_CHAN, 4096, 16000.0), IRIS_OK, "8 channels: the unset microphones sit in the corner (0, 0, 0), inside the room");
    expect(iris_ism_rir(nullptr, nullptr, 0, 2, 4096, 16000.0, 1, nullptr), IRIS_OK, "empty table");
    expect(iris_ism_rir(t.data(), dev, -1, 2, 4096, 16000.0, 1, nullptr), IRIS_E_INVALID, "n_src < 0");
    expect(iris_ism_rir(t.data(), dev, 3, 0, 4096, 16000.0, 1, nullptr), IRIS_E_INVALID, "channels = 0");
    expect(iris_ism_rir(t.data(), dev, 3, 9, 4096, 16000.0, 1, nullptr), IRIS_E_UNSUPPORTED, "channels = 9");
    expect(iris_ism_rir(nullptr, dev, 3, 2, 4096, 16000.0, 1, nullptr), IRIS_E_INVALID, "NULL host table");
    expect(iris_ism_rir(t.data(), dev, 3, 2, 4097, 16000.0, 1, nullptr), IRIS_E_INVALID, "max_taps > 4096");
    expect(iris_ism_rir(t.data(), dev, 3, 2, 63, 16000.0, 1, nullptr), IRIS_E_INVALID, "max_taps < K");
    expect(iris_ism_rir(t.data(), dev, 3, 2, 4096, NAN, 1, nullptr), IRIS_E_INVALID, "sample rate NaN");
    const double huge = 1e308, nan = NAN, inf = INFINITY;
    for (int field = 0; field < 12; ++field) {
        iris_ism_src r = good();
        switch (field) {
            case 0: r.n_taps = 0; break;
            case 1: r.n_taps = INT_MAX; break;
            case 2: r.room[1] = 0; break;
            case 3: r.room[2] = inf; break;
            case 4: r.room[0] = nan; break;
            case 5: r.src[0] = 3.2; break;
            case 6: r.src[2] = nan; break;
            case 7: r.mic[1][1] = -huge; break;
            case 8: r.beta = 1.0; break;
            case 9: r.beta = nan; break;
            case 10: memcpy(r.src, r.mic[1], sizeof r.src); break;                      // on the nearest microphone
            default:                                                                     // a lattice beyond 2^31 - 1 images
                r.room[0] = r.room[1] = r.room[2] = 1e-300, r.n_taps = 4096;
                for (int a = 0; a < 3; ++a) r.src[a] = 5e-301, r.mic[0][a] = 2e-301, r.mic[1][a] = 3e-301;
        }
        t[2] = r;
        char what[32];
        snprintf(what, sizeof what, "bad field %d", field);
        expect(iris_ism_rir(t.data(), dev, 3, 2, 4096, 16000.0, 1, nullptr), IRIS_E_INVALID, what);
        if (!strstr(iris_last_error(), "record 2")) printf("FAIL %s: %s\n", what, iris_last_error()), ++failures;
    }
    printf(failures ? "%d check(s) failed\n" : "ism_args_check: all checks passed%.0d\n", failures);
    return failures != 0;
}
