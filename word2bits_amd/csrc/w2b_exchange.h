// w2b_exchange.h -- the replica exchange (w2b_exchange.cpp) as the trainer (w2b_trainer.cpp) sees it.  A W2bExchange owns the
// communicator, the two exchange streams, the staging buffers, `base` and the per-row counts and rates; it exists from
// w2b_comm_init / w2b_exchange_init on (w2b_trainer::xchg, null before) and reads the trainer through W2bExchangeView alone.
// The trainer reaches it through the five operations below; each accepts a null exchange and then does nothing.  Internal.
#pragma once
#include "w2b_plan.h"

struct W2bExchangeView {
  float *uv;                   // [u || v]
  long long table_elems;       // floats of one table
  hipStream_t stream;          // the training stream
  W2bShared *shared;
  const W2bPlanInputs &in;     // configuration, tuning knobs, word-count statistics
};
struct W2bExchange;

// The training stream (and with it every reader of the model) waits for the exchange in flight; *waited: there was one, so
// the model may have changed under the caller.
int w2b_xchg_fence(W2bExchange *x, bool *waited);
hipError_t w2b_xchg_rebase(W2bExchange *x, hipStream_t s);   // base := model on s (the model was replaced: w2b_init_net, w2b_set_model)
void w2b_xchg_add_words(W2bExchange *x, long long words);    // centre words trained since the previous exchange (the n of the combination rule)
int w2b_xchg_upload_rates(W2bExchange *x);                   // the word counts of the view have changed: per-row update rates
void w2b_xchg_destroy(W2bExchange *x);                       // synchronises the exchange streams, then releases everything
