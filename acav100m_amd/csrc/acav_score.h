// acav_score.h -- subset scoring (acav_score.hip), called from the MI handle's entry point in acav_mi.hip
#pragma once
#include "acav_common.h"

namespace acav {

// everything acav_mi_score_subset has validated and put on the device; nothing of the handle's tables is in here
struct ScoreJob {
    int device = 0;
    hipStream_t stream = nullptr;
    const int *asg = nullptr;    // [V, D] labels
    const int *pairs = nullptr;  // [P, 2] column indices
    int64_t V = 0;
    int D = 0, C = 0, P = 0;
    const int *ids = nullptr;    // [n] ids, every one inside [0, V)
    int64_t n = 0;
    const int64_t *prefix = nullptr;  // host, [nprefix], strictly increasing, ends at n
    int nprefix = 0;
    unsigned mask = 0;
    const double *lnk = nullptr, *lf = nullptr;  // ln k and ln k! for k <= max(V + 1, n)
    double *scores = nullptr;             // host [nprefix][6]
    double *per_pair = nullptr;           // host [nprefix][6][P] or NULL
    acav_score_stats *stats = nullptr;    // host [nprefix][P] or NULL
};

// builds the tables of the job's own, scores every prefix, one host synchronisation
int score_subset_run(const ScoreJob &job);

}  // namespace acav
