// LocalBA: what the test taps (csrc/lba_taps.hip) share with the solve (csrc/lba_solve.hip) -- the handle's cache and streams and
// the host phase of a call up to the upload.  Internal to the library.
#pragma once
#include "lba_launch.h"

namespace aos2 {

// host-side structure buffers and worker threads of a handle, kept between calls (aos2_lba::lba_cache)
struct LbaCache {
    std::vector<Pass> passes;
    WindowPool pool;
};

// the streams of window group g (the second group's exist once a call ran two groups)
StreamSet group_streams(const aos2_lba *s, int g);

// The host phase of a call up to the upload (aos2_lba_solve_batch and the taps share it): the index structures of the windows
// `act` (a pool thread per window), the task lists of the G groups, the arena, staging + upload, the descriptors
struct Uploaded {
    std::vector<Pass> *passes = nullptr;   // the handle's (LbaCache)
    TaskLists TL[2];
    ArenaPlan A;
    LbaWin *hw = nullptr;                  // the host's copy of the descriptors
    GroupDims gd[2];
    DevTasks dt[2];
    int max_i1 = 0, max_i2 = 0;
    bool any_flag = false;
};
int build_and_upload(aos2_lba *s, const aos2_lba_problem_t *problems, const std::vector<int> &act, const int (&goff)[3], int G, const LmLayout &lay,
                     bool want_chi2, Uploaded &U);

}  // namespace aos2
