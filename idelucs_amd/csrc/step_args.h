// step_args.h -- host-side checks of the argument structs that the LAST launch of a training step takes, whichever optimizer ends it
// (idl_rmsprop_step in train_step.hip, idl_opt_step_gather_wgrad in opt_step.hip, idl_small_wgrad_* in small_step.hip): one text for the
// next batch an optimizer launch assembles and one for an optimizer's state.  Every check stands before the first HIP call; a refusal
// names the caller and the field.  (train_step.hip's riders_of is the counterpart for the middle launches, which assemble shares.)
#pragma once
#include "common.h"
#include "scaler_device.h"

namespace idl_step {

inline int refuse(const char *who, const char *what)      // (IDL_REQUIRE's message, the caller named)
{
    idl::set_error("bad argument: %s: %s", who, what);
    return IDL_ERR_ARG;
}

// The next batch as an optimizer launch assembles it: the WHOLE batch, fp32 rows only, at the offset ctl[1] that an earlier launch of the step
// advanced.  nb == NULL (or nb->feats == NULL): out.y stays NULL, no assembly.
inline int whole_batch_of(const char *who, const idl_next_batch_t *nb, const int64_t *ctl, idl_dev::GatherArgs &out)
{
    out = idl_dev::GatherArgs{};
    if (nb == nullptr || nb->feats == nullptr) return IDL_OK;
    if (!(ctl != nullptr && nb->base == ctl + 1)) return refuse(who, "the optimizer launch assembles the batch at ctl[1]: next_batch->base must be ctl + 1");
    if (!(nb->y_hi == nullptr && nb->y_lo == nullptr)) return refuse(who, "the optimizer launch writes no planes of the next batch");
    if (nb->base_add != 0) return refuse(who, "the optimizer launch takes no base_add");
    if (!(nb->part == 0 && nb->part_end == nb->parts)) return refuse(who, "the optimizer launch assembles the whole batch, not a share");
    if (!(nb->pair_idx && nb->mean && nb->scale && nb->y && nb->n >= 1 && nb->f >= 1 && nb->batch >= 1 && nb->n_pairs >= 0)) return refuse(who, "bad gather arguments");
    out = idl_dev::GatherArgs{nb->feats, nb->n, nb->f, nb->view_stride, nb->pair_idx, ctl + 1, nb->batch, nb->n_pairs, nb->mean, nb->scale, nb->inv_scale, nb->y};
    out.wt = idl_store::wt_mask();
    return IDL_OK;
}

// idl_opt_state_t of a launch over n_tensors tensors whose counters are ctl[0..1]; kinds_allowed: bit k set = kind k is taken.
inline int opt_state_of(const char *who, const idl_opt_state_t *opt, const int64_t *ctl, unsigned kinds_allowed, int n_tensors)
{
    if (opt == nullptr) return refuse(who, "NULL opt");
    if (!(opt->kind >= 1 && opt->kind <= 3 && ((kinds_allowed >> opt->kind) & 1u)))
        return refuse(who, (kinds_allowed >> 3) & 1u ? "opt->kind is 1 (SGD with momentum), 2 (Adam) or 3 (RMSprop with momentum)" : "opt->kind is 1 (SGD with momentum) or 2 (Adam)");
    if (opt->state1 == nullptr || (opt->kind != 1 && opt->state2 == nullptr))
        return refuse(who, "opt->state1 is needed, and opt->state2 for Adam (exp_avg_sq) and RMSprop (momentum_buffer)");
    for (int t = 0; t < n_tensors; ++t)
        if (opt->state1[t] == nullptr || (opt->kind != 1 && opt->state2[t] == nullptr)) return refuse(who, "NULL entry in opt->state1 / opt->state2");
    if (opt->hyper == nullptr || (((uintptr_t)opt->hyper) & 7u) != 0) return refuse(who, "opt->hyper is a device double[5]");
    if (!(opt->step_in && opt->step_out && opt->step_in != opt->step_out))
        return refuse(who, "opt->step_in / opt->step_out: the step count is read from one word and written to another");
    if (ctl != nullptr && (opt->step_in == ctl || opt->step_in == ctl + 1)) return refuse(who, "opt->step_in must not be a word this launch writes");
    return IDL_OK;
}

}  // namespace idl_step
