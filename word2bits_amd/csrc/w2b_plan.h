// w2b_plan.h -- the launch policy of the library (w2b_plan.cpp): which worker kernel runs, which rows get per-XCD copies,
// lossless adds or refreshed read copies, the merge period, how many workers run at once.  Host arithmetic on the
// configuration, the tuning knobs and the word counts; the trainer (w2b_trainer.cpp) asks for a W2bLaunchPlan once per launch
// and applies it.  Internal, like w2b_internal.h.
#pragma once
#include "../../include/word2bits_hip.h"
#include "w2b_internal.h"

#include <vector>

// Everything the policy reads.  A trainer holds one (w2b_trainer::in); w2b_plan_rows fills one without a device.
struct W2bPlanInputs {
  w2b_config cfg{};
  w2b_tuning tune{};                    // knobs of include/word2bits_hip.h (w2b_default_tuning until w2b_set_tuning)
  int num_cus = 0;
  // the word-count statistics (w2b_plan_set_counts; empty / 0 = no word counts yet)
  std::vector<int64_t> counts;          // vocab[].cn as given to w2b_set_vocab_counts (sorted by count behind row 0)
  double counts_pw = 0, counts_tot = 0; // sum cn^0.75, sum cn
  double counts_tot_kept = 0;           // sum of the expected KEPT occurrences (sub-sampling, ref :403-406)
  std::vector<double> rate_v, rate_u;   // [k]: uses of row k + 1 of v (as a target) / of u (as a context row) per centre word
};

enum { W2B_KERNEL_PLAIN = 0, W2B_KERNEL_RESIDENT = 1, W2B_KERNEL_GROUPS = 2 };   // (the numbers w2b_worker_kernel_info reports)

// Every decision of one launch.
struct W2bLaunchPlan {
  int kernel;                 // W2B_KERNEL_*
  int radius;                 // sentence-resident kernel: the window radius it keeps in LDS; -1 for the other two
  int copies_u, copies_v;     // rows 1..N of u / v with per-XCD copies
  int uavg_rank;              // sentence-resident kernel: context rows 1..N merged by consensus and refreshed
  int atomic_rank_v, atomic_rank_u;   // rows 1..N of v / u updated by lossless adds
  int fresh_rank_u;           // plain kernels: context rows 1..N re-read before their update
  int merge_period;           // centre words between two merge events of a worker
  int xhot_m;                 // rows with copies that one merge event brings up to date
  int refresh_rows_u;         // row-group kernel: context rows 1..N read at refreshed per-XCD copies
  int concurrent_workers;     // plain kernel: workers that run at once (= workers for the other two)
  int full_device;            // 1: the launch has at least W2B_FULL_DEVICE_WG_PER_CU workgroups per CU
};

w2b_tuning w2b_default_tuning();
// word counts -> the statistics of `in`; returns the sub-sampling keep table (w2b_build_keep_prob; all 1 without sub-sampling)
std::vector<float> w2b_plan_set_counts(W2bPlanInputs &in, const int64_t *cn);
// plain_only: plan as if w2b_config.plain_worker_kernel were 1 (the tuple form, which has no other kernel)
W2bLaunchPlan w2b_plan_launch(const W2bPlanInputs &in, long long workers, bool plain_only = false);
// w2b_suggested_threads: the worker count its kernel choice is judged at, and what to suggest when `device_workers` workers
// (workgroups per CU of the kernel that would run x CUs) fit on the device
long long w2b_plan_probe_workers(const W2bPlanInputs &in);
long long w2b_plan_suggested_workers(const W2bPlanInputs &in, const W2bLaunchPlan &probe, long long device_workers);
// expected KEPT occurrences of a word with count c (sub-sampling, ref :403-406), and the uses of a row of v with count c as a
// target per centre word (negative draws on the raw counts, ref :112-128, + the centre word itself)
double w2b_plan_kept(const W2bPlanInputs &in, double c);
double w2b_plan_rate_v(const W2bPlanInputs &in, double c);
