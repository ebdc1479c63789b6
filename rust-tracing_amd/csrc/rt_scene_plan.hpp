// rt_scene_plan.hpp — everything rt_scene_create_ex decides and every byte it uploads, computed without a device: the host compiler
// builds rt_scene_plan.cpp, which calls no hip* function and needs neither the HIP runtime nor rt_kernel.o (rt_kernels.h gives it the
// types and constants).  rt_api.cpp uploads a plan and launches from its Layout; rt_debug_scene_plan (rt_debug.cpp) shows one;
// tools/sanitize/fuzz_scene_compiler.cpp runs it under the sanitizers.
#pragma once
#include "rt_amd.h"
#include "rt_compile.hpp"
#include "rt_kernels.h"
#include "rt_ordered.hpp"

#include <string>
#include <vector>

namespace rtapi {
using namespace rtd;
using namespace rtk;

int fail(int status, const std::string &msg); // sets rt_last_error() of the calling thread, returns `status`

// Scheduler knobs (64ths of the live lanes a deferred stage must have queued / the box loop needs to keep running).
// The best values depend on the stage mix, so there is one preset per kernel instantiation, each picked with
// tools/tune.py on MI355X (DESIGN.md "Scheduler"); a value >= 0 in `forced` (RT_TH_* variables, rt_debug_set_tuning)
// overrides all presets.
struct Thresholds { uint32_t prim, other, shade, box, newjob; };
struct Tuning {
    Thresholds general{8, 8, 48, 8, 0};
    Thresholds ordered_general{8, 12, 40, 8, 0}; // every feature, ordered walk (final_scene: 760 vs 745 Msamples/s at 60 spp)
    Thresholds ordered_global{4, 8, 48, 8, 0};   // ... the same walk with the scene gathered from global memory (final_scene; swept twice on round 3's kernels: +0.4 % over the
                                                // preset above, which stays for the LDS-resident scenes — cornell_smoke loses 5 % with this one)
    Thresholds spheres_solid{6, 16, 32, 6, 28};  // random-spheres (re-tuned with the start shortcut: 5070 vs 4900 Msamples/s at 50 spp for round 1's 8/16/24/16/32)
    Thresholds quads_frames{24, 16, 48, 2, 0}; // Cornell box (tools/tune.py; with instances walked last and flat leaves the merged path end wins: round 1's 8/16/40/4/8 is 7 % behind)
    Thresholds spheres_threaded{8, 16, 24, 16, 32}; // ... the same kernel walking the reference's order (no shortcut there)
    Thresholds quads_only{8, 16, 40, 4, 8};    // ... the same kernel on a scene without instances (quads: 13.4 vs 12.8 Gsamples/s with the preset above)
    int forced[5] = {-1, -1, -1, -1, -1};    // prim, other, shade, box, newjob
    int use_lds = 1; // 0: always gather the scene from global memory (tuning / A-B runs)
    int refit = 1;   // 0: walk the reference's own (looser) boxes
    int ordered = 1; // scenes created from now on: 0 always the reference-order walk, 1 the ordered walk where it pays
                     // (ordered_walk_pays), 2 the ordered walk wherever the scene allows it
    int jobs_per_grab = 0; // > 0: fixed grab size (RT_JOBS_PER_GRAB; tuning runs)
    int wide = -1;         // own trees with four-child records (rt_layout.h ONode4): 1 always, 0 never, -1 for scenes of 64 primitives or more (RT_WIDE)
    int wide_setaside = 1; // four-child records: 1 = the one inner child left to look at is set aside as itself, 0 = as its record with a one-bit mask (RT_WIDE_SETASIDE)
    int quad_filter = 1;   // multi-quad leaves go through the conservative f32 filter before the exact test (RT_QUAD_FILTER; rt_scene_options.quad_filter)
    int medium_first = 1;  // a ray that starts inside a sphere-bounded medium: that medium's draw first, the tree in front of it clipped (RT_MEDIUM_FIRST)
    int overlap = 1;       // 1: a frame of several launches alternates between two scratch sets on two streams (RT_OVERLAP)
    int slow_min = 4, slow_age = 32; // KParams::slow_min / slow_age (RT_SLOW_MIN, RT_SLOW_AGE; slow_min 1: nobody waits)
    int seq_lookahead = 1;  // scenes with media: a query looks ahead at the boxes of the sequence's later steps when it starts (RT_SEQ_LOOKAHEAD)
    int start_shortcut = 1; // a root whose one child is a single sphere spanning the scene (random-spheres' ground): queries start with that sphere's test (RT_START_SHORTCUT)
    int start_inline = 1;   // ... and where that leaf is one sphere, its test runs where the query starts, not in a round of the sphere stage (RT_START_INLINE; rt_debug_set_start_inline)
    int defer = 1;         // ordered walk: the world frame's instances (<= 32) are walked after the world's own tree, one frame change each instead of two (RT_DEFER)
    int grab_taper = 8;    // guided hand-out: a grab takes at most 1 / (waves x this) of the jobs left (RT_GRAB_TAPER; 0: off; tools/sweep_grabs.sh)
    OrderedOptions ordered_options;
    size_t sample_buffer_bytes = (size_t)2 << 30; // per-(scene, stream) sample buffer at most (halved on out-of-memory)
    Tuning();
    Thresholds pick(const Thresholds &preset) const {
        Thresholds t = preset;
        if (forced[0] >= 0) t.prim = (uint32_t)forced[0];
        if (forced[1] >= 0) t.other = (uint32_t)forced[1];
        if (forced[2] >= 0) t.shade = (uint32_t)forced[2];
        if (forced[3] >= 0) t.box = (uint32_t)forced[3];
        if (forced[4] >= 0) t.newjob = (uint32_t)forced[4];
        return t;
    }
};

// The tree-building options a scene gets from its (resolved) options on top of the process defaults: leaf_max and flat_max.  `wide` is
// the caller's to set — compile_for_scene decides it from the compiled scene's size, the layout hooks of rt_debug.cpp force it.
OrderedOptions ordered_options_for(const rt_scene_options &opt, const Tuning &tn);
// The scene as rt_scene_create_ex compiles it under `opt` (already resolved) and the process defaults `tn` (RT_* variables,
// rt_debug_set_*): which walk, which boxes, which records.  Shared with rt_debug_wide_records, so that the hook shows what a scene gets.
int compile_for_scene(const rt_scene_desc &desc, const rt_scene_options &opt, const Tuning &tn, CompiledScene &cs, const char *who);
float ordered_box_extent(const CompiledScene &cs); // Layout::box_extent, as scene creation computes it

// A scene's node tables as the device holds them.  `tables`: the LDS form, plane tables of table_bytes each and the reference table behind
// them — two 16-byte halves per threaded record; six plane tables X+ | X- | Y+ | Y- | Z+ | Z- and references for the library's own trees
// (16 + 8 bytes per two-child record, rt_device_scene.h load_opair; 32 + 16 per four-child record, load_oquad: the planes a ray of that sign
// enters the four children through, then the four it leaves them through).  `lines`: the global form of the own trees' tables — a record's
// seven pieces side by side in 128 bytes (two children) or 256 (four: offsets 0 .. 160, 192).  One function for the plan and the hooks of
// rt_debug.cpp, so that what a test inspects or feeds to the kernel is what a scene uploads.
struct NodeTables {
    std::vector<uint4> tables, lines;
    size_t table_bytes = 0; // KParams::lds_off_node_b
    size_t records = 0;
};
NodeTables pack_wide_records(const std::vector<ONode4> &recs);

struct ScenePlan {
    // Where a query starts (KParams::o_start_*): the stage of the start leaf's kind (0: at the root), its primitives [prim, end), what is set
    // aside (two children: the root's other child; four: the mask of the root's other children), the leaf's slot in the root
    struct Start {
        uint32_t stage = 0, prim = 0, end = 0, rest = 0, slot = 0;
        uint32_t direct = 0xffffffffu; // wide: the root's one other child if that is an inner record (its index), else none
    };
    struct Lds { // the LDS image: node tables | spheres | quads | quad filter records; every LDS level copies a prefix
        int level = 0;                // 0 nothing fits, 1 nodes, 2 nodes + spheres, 3 nodes + spheres + quads
        uint32_t off_node_b = 0, off_spheres = 0, off_quads = 0;
        uint32_t off_qfilt = 0;       // the quads' f32 filter records in the LDS image (0: none)
        uint32_t prefix_bytes[4] = {0, 0, 0, 0}; // image prefix each LDS level copies in
    };
    struct Aux { // materials | textures | frames | media | Perlin for the AUX kernels (0 bytes: not used)
        uint32_t bytes = 0, off[5] = {0, 0, 0, 0, 0};
    };
    // The scalars.  walk_layout() fills the first block; the LDS helpers below up to stack_bytes read nothing else.
    struct Layout {
        uint32_t features = F_ALL;  // Feature bits the scene uses
        bool parks_colours = false; // some attenuation is a texture's value: launches need the colour stack (KParams::att_stack)
        bool has_instances = false;
        bool ordered = false;       // ordered layout (rt_ordered.hpp): onodes instead of nodes
        bool wide = false;          // ... with four-child records (onodes4)
        uint32_t o_root = 0, o_stack = 0; // world root record; stack entries per lane
        uint32_t n_oseq = 0, n_nodes = 0;
        float box_extent = 0.0f;    // largest |coordinate| of any box of the ordered layout
        Start start;
        Lds lds;
        Aux aux;
    };
    Layout layout;
    rt_scene_stats stats{};
    std::vector<uint4> oimage;       // ordered layout: the node tables' global form (empty: the reference-order walk)
    std::vector<uint4> lds_image;    // empty: LDS level 0
    std::vector<uint4> aux_image;    // empty: no AUX kernels for this scene
    std::vector<DMaterial> mats;
    CompiledScene cs;                // the tables uploaded as they are (instances carry their start_ref / start_box)
};
// The plan of the scene rt_scene_create_ex makes of `desc` under `resolved` options and the process defaults `tn`.  No exception leaves
// it: what compile_for_scene refuses keeps its status and message, std::bad_alloc gives RT_ERR_OUT_OF_MEMORY.
int plan_scene(const rt_scene_desc &desc, const rt_scene_options &resolved, const Tuning &tn, ScenePlan &out, const char *who);

// ---- the dynamic LDS of a launch at LDS level `lds` (0, or the scene's level): NORMATIVE for the plan and the launch alike ----
// image prefix | per-lane stacks (ordered walk: 2-byte entries beside an LDS-resident scene, else 4-byte) | the world's sequence |
// the small tables (AUX kernels) | parked world rays | profile rows — each region 16-byte aligned; the optional parts are taken in
// this order for as long as the CU's LDS has room (the instrumented kernel's rows included, so that it has the layout of the one it
// stands in for)
using Layout = ScenePlan::Layout;
inline size_t align16(size_t x) { return (x + 15u) & ~(size_t)15u; }
inline int block_threads(const Layout &l, int lds) { return kernel_threads_for(kernel_features_for(l.features, lds, l.ordered), lds, l.ordered); }
inline size_t stack_bytes(const Layout &l, int lds) {
    if (!l.ordered) return 0;
    return (size_t)l.o_stack * (size_t)block_threads(l, lds) * (lds ? 2u : 4u);
}
inline size_t prof_bytes(const Layout &l, int lds) { return (size_t)(block_threads(l, lds) / 64) * PROF_SLOTS * 3u * sizeof(unsigned long long); }
inline size_t seq_offset(const Layout &l, int lds) { return align16(l.lds.prefix_bytes[lds] + stack_bytes(l, lds)); }
inline size_t aux_offset(const Layout &l, int lds) { return align16(seq_offset(l, lds) + (l.ordered ? (size_t)l.n_oseq * sizeof(OSeq) : 0u)); }
inline bool aux_in_lds(const Layout &l, int lds) {
    return l.ordered && l.aux.bytes != 0 && aux_offset(l, lds) + l.aux.bytes + prof_bytes(l, lds) <= LDS_BUDGET_BYTES;
}
inline size_t world_offset(const Layout &l, int lds) { return align16(aux_offset(l, lds) + (aux_in_lds(l, lds) ? l.aux.bytes : 0u)); }
inline size_t world_bytes(const Layout &l, int lds) { return (size_t)6 * sizeof(double) * (size_t)block_threads(l, lds); }
inline bool world_in_lds(const Layout &l, int lds) {
    return l.has_instances && world_offset(l, lds) + world_bytes(l, lds) + prof_bytes(l, lds) <= LDS_BUDGET_BYTES;
}
inline size_t prof_offset(const Layout &l, int lds) { return world_offset(l, lds) + (world_in_lds(l, lds) ? world_bytes(l, lds) : 0u); }
inline size_t dynamic_lds_bytes(const Layout &l, int lds, bool counted) { return prof_offset(l, lds) + (counted ? prof_bytes(l, lds) : 0); }
// rt_scene::blocks_per_cu's second index: every instantiation a render may launch has its own occupancy figure (only the dense
// kernel has an instrumented twin)
inline int kernel_variant(bool counted, int jobs) { return jobs == JOBS_VIEWS ? 3 : jobs == JOBS_LIST ? 2 : counted ? 1 : 0; }

} // namespace rtapi
