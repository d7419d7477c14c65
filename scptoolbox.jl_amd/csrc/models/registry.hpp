// The compiled models of the library, listed ONCE: the dispatch from a model id (include/scp_mi355x.h) to the model type, and the
// subsets every unit derives from it -- the models with the structured PTR fast path, the models the audits are defined for, and the
// (nx, nu) pairs the packed chains of the audits are instantiated for.  A new model is a header, an id and a line of with_model.
#pragma once
#include "../../../include/scp_mi355x.h"
#include "double_integrator.hpp"
#include "quadrotor.hpp"
#include "rocket_landing.hpp"
#include "starship.hpp"
#include "freeflyer.hpp"
#include "oscillator.hpp"

namespace scp {

// dispatch a generic lambda on the model type
template <class Fn>
static int with_model(int model_id, Fn&& fn)
{
    switch (model_id) {
        case SCP_MODEL_DOUBLE_INTEGRATOR: return fn(DoubleIntegrator{});
        case SCP_MODEL_QUADROTOR: return fn(Quadrotor{});
        case SCP_MODEL_ROCKET_LANDING: return fn(RocketLanding{});
        case SCP_MODEL_STARSHIP: return fn(Starship{});
        case SCP_MODEL_FREEFLYER: return fn(Freeflyer{});
        case SCP_MODEL_OSCILLATOR: return fn(Oscillator{});
        default: return SCP_ERR_UNKNOWN_MODEL;
    }
}
// models with the stage-structured PTR fast path (stage_problem.hpp + ipm2_*.hpp: one arrow column, <= 16 penalised rows
// per node); the others (M::structured == false) run their subproblems through the generic conic path
template <class Fn>
static int with_structured_model(int model_id, Fn&& fn)
{
    return with_model(model_id, [&](auto m) -> int {
        if constexpr (decltype(m)::structured) return fn(m);
        else return (int)SCP_ERR_UNSUPPORTED;
    });
}

// the models the audits are defined for: no node parameters.  A row of X at node k reads that node's own slack (the free-flyer's
// room slacks, the oscillator's one-norm slack), and between the nodes, where the audits sample, no slack exists
template <class M>
constexpr bool auditable = M::np_node == 0;

template <class Fn>
static int with_auditable_model(int model_id, Fn&& fn)
{
    return with_model(model_id, [&](auto m) -> int {
        if constexpr (auditable<decltype(m)>) return fn(m);
        else return (int)SCP_ERR_UNSUPPORTED;
    });
}

// fn(Chain<nx, nu>{}) for the first auditable model of these dimensions: a packed chain (Lqr, Cov) exists for the pairs of the
// auditable models and for no other, and its own static_assert refuses a model too wide for it.  The ids are consecutive from 0
template <template <int, int> class Chain, class Fn>
static int with_auditable_dims(int nx, int nu, Fn&& fn)
{
    for (int id = 0;; id++) {
        bool found = false;
        const int rc = with_model(id, [&](auto m) -> int {
            using M = decltype(m);
            if constexpr (auditable<M>) {
                if (M::nx == nx && M::nu == nu) { found = true; return fn(Chain<M::nx, M::nu>{}); }
            }
            return (int)SCP_OK;
        });
        if (found) return rc;
        if (rc == SCP_ERR_UNKNOWN_MODEL) return (int)SCP_ERR_UNSUPPORTED;
    }
}

}  // namespace scp
