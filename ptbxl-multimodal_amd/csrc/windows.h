// windows.h — the window rule and the grid limits of the input step, shared by input.hip and fir.hip.
#pragma once
#include "common.h"

namespace ecg {

constexpr int kMaxLeads = 16;

// Where the windows of a launch lie in their recordings d [R][Ttot][leads]: window b = r*W + w of the
// grid starts at sample first + w*hop of recording r — or at last_start when that is >= 0 and w is the
// last window (the "shifted tail" that ends with the recording).  Pre-cut windows [B][T][leads] are the
// case Ttot == T, W == 1.  A start is any sample index: the source is only ever read as int16.
struct WindowSrc {
    long long Ttot;
    int W, first, hop, last_start;
};

__device__ __forceinline__ long long window_start(const WindowSrc &s, int w) {
    return (s.last_start >= 0 && w == s.W - 1) ? (long long)s.last_start : s.first + (long long)w * s.hop;
}

// The window rule on the host: every start inside [0, Ttot - T], checked before any launch.
static int check_windows(const char *who, int R, int Ttot, int T, int first, int hop, int W, int last_start) {
    ECG_REQUIRE(R > 0 && T > 0, "%s: R=%d T=%d must be > 0", who, R, T);
    ECG_REQUIRE(hop >= 1 && W >= 1, "%s: hop=%d W=%d must be >= 1", who, hop, W);
    ECG_REQUIRE(T <= Ttot, "%s: window T=%d longer than the recording Ttot=%d", who, T, Ttot);
    ECG_REQUIRE(last_start >= -1 && last_start <= Ttot - T, "%s: last_start=%d outside [-1, Ttot-T=%d]", who,
                last_start, Ttot - T);
    const int wreg = last_start >= 0 ? W - 1 : W;       // windows on the first + w*hop lattice
    ECG_REQUIRE(first >= 0, "%s: first=%d must be >= 0", who, first);
    ECG_REQUIRE(wreg == 0 || first + (long long)(wreg - 1) * hop <= Ttot - T,
                "%s: window %d starts at %lld, past Ttot-T=%d", who, wreg - 1, first + (long long)(wreg - 1) * hop,
                Ttot - T);
    return ECG_OK;
}

// The grid limits of a window launch: leads in range, one grid.y row per window (NW = R*W) and, when ecg_zscore_rows
// takes the statistics of the result (`rows`), one per (window, lead).
static int check_grid(const char *who, int leads, long long NW, bool rows, int T) {
    ECG_REQUIRE(leads >= 1 && leads <= kMaxLeads, "%s: leads=%d outside [1,%d]", who, leads, kMaxLeads);
    ECG_REQUIRE(NW <= 65535, "%s: %lld windows exceed grid.y limit 65535", who, NW);
    ECG_REQUIRE(!rows || NW * leads <= 65535, "%s: windows*leads=%lld exceeds 65535 rows for T=%d", who, NW * leads, T);
    return ECG_OK;
}

}  // namespace ecg
