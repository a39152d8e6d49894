// vmv_plans.h — the result object of the planning calls (vmv_rrtc_multi, vmv_prm_multi, vmv_aorrtc_multi, vmv_fcit_multi, vmv_roadmaps_query): vmv_plans_summary,
// vmv_plans_paths and vmv_plans_destroy (vmv_rrtc_multi.hip) read the first block whichever call made it.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include <vector>

struct vmv_plans
{
    size_t n = 0;
    int dim = 0;
    std::vector<uint8_t> status;
    std::vector<uint32_t> iterations, sizes2, path_lengths;
    std::vector<float> paths;  // packed in problem order
    uint64_t rounds = 0, questions = 0;

    // vmv_rrtc_multi_goals only (vmv_plans_goal_indices)
    bool rrtc_goals = false;
    std::vector<uint32_t> goal_indices;  // [n] the goal, within its own set, a solved path ends in; UINT32_MAX = unsolved

    // vmv_rrtc_multi_constrained and vmv_aorrtc_multi_constrained only (vmv_plans_band_refused)
    bool constrained = false;
    std::vector<uint32_t> band_refused;  // [n] questions the constraint answered 0 (projection or band test), all stages

    // vmv_prm_multi only (vmv_plans_roadmap_*)
    bool prm = false, kept = false;  // made by vmv_prm_multi; with keep_roadmaps
    uint32_t n_samples = 0;
    std::vector<uint32_t> candidate_edges;  // [n]
    std::vector<float> costs;               // [n]
    std::vector<uint8_t> vertex_valid;      // kept: [n][n_samples + 2]
    std::vector<uint32_t> edge_offsets;     // kept: [n + 1] first candidate edge of each problem
    std::vector<uint32_t> edge_pairs;       // kept: [edges][2] vertex ids a < b, in candidate order
    std::vector<uint8_t> edge_valid;        // kept: [edges]

    // vmv_aorrtc_multi and vmv_aorrtc_multi_constrained only (vmv_plans_costs)
    bool aorrtc = false;
    std::vector<float> first_costs, final_costs;  // [n] after the first stage; of the returned path (+inf = unsolved)
    std::vector<uint32_t> searches, improvements; // [n] cost-bounded searches run; those that gave a cheaper path

    // vmv_fcit_multi only (vmv_plans_fcit_summary; n_samples and costs as above)
    bool fcit = false;
    std::vector<uint32_t> known_valid;  // [n] edges the walk found valid

    // vmv_roadmaps_query only (vmv_plans_query_summary; costs as above, candidate_edges = the questions a query asked)
    bool query = false;
};
