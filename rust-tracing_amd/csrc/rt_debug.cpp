// rt_debug.cpp — the test and tuning hooks of include/rt_amd_debug.h (not part of the drop-in boundary).
#include "rt_api.hpp"
#include "rt_qfilt.hpp"

#include <cmath>
#include <cstring>

using namespace rtapi;

extern "C" {

int rt_debug_set_tuning(int32_t th_prim, int32_t th_other, int32_t th_shade, int32_t th_box, int32_t use_lds, int32_t th_new) {
    const int32_t v[6] = {th_prim, th_other, th_shade, th_box, th_new, use_lds};
    tuning_update([](Tuning &t, const void *arg) {
        const int32_t *a = static_cast<const int32_t *>(arg);
        for (int k = 0; k < 5; ++k) t.forced[k] = a[k];
        if (a[5] >= 0) t.use_lds = a[5];
    }, v);
    return RT_OK;
}

int rt_debug_set_traversal(int32_t ordered, int32_t leaf_max) {
    const int32_t v[2] = {ordered, leaf_max};
    tuning_update([](Tuning &t, const void *arg) {
        const int32_t *a = static_cast<const int32_t *>(arg);
        if (a[0] >= 0) t.ordered = a[0];
        if (a[1] > 0) t.ordered_options.leaf_max = (uint32_t)a[1] < OREF_MAX_LEAF ? (uint32_t)a[1] : OREF_MAX_LEAF;
        else if (a[1] == 0) t.ordered_options.leaf_max = OrderedOptions().leaf_max;
    }, v);
    return RT_OK;
}

int rt_debug_set_walk_shortcuts(int32_t flat_max, int32_t start_shortcut, int32_t defer_instances, int32_t seq_lookahead, int32_t slow_min,
                                int32_t slow_age) {
    const int32_t v[6] = {flat_max, start_shortcut, defer_instances, seq_lookahead, slow_min, slow_age};
    tuning_update([](Tuning &t, const void *arg) {
        const int32_t *a = static_cast<const int32_t *>(arg);
        if (a[0] >= 0) t.ordered_options.flat_max = (uint32_t)a[0];
        if (a[1] >= 0) t.start_shortcut = a[1];
        if (a[2] >= 0) t.defer = a[2];
        if (a[3] >= 0) t.seq_lookahead = a[3];
        if (a[4] >= 1) t.slow_min = a[4];
        if (a[5] >= 0) t.slow_age = a[5];
    }, v);
    return RT_OK;
}

int rt_debug_set_start_inline(int32_t start_inline) {
    tuning_update([](Tuning &t, const void *arg) {
        const int32_t v = *static_cast<const int32_t *>(arg);
        if (v >= 0) t.start_inline = v;
    }, &start_inline);
    return RT_OK;
}

int rt_debug_ordered_layout(const rt_scene_desc *desc, rt_debug_ordered *io) { return rt_debug_ordered_layout_ex(desc, nullptr, io); }

int rt_debug_ordered_layout_ex(const rt_scene_desc *desc, const rt_scene_options *options, rt_debug_ordered *io) {
    if (!desc || !io) return fail(RT_ERR_INVALID_ARGUMENT, "rt_debug_ordered_layout: null argument");
    rt_scene_options opt; // (checked and defaulted exactly as rt_scene_create_ex does)
    if (int orc = resolve_scene_options(options, opt, "rt_debug_ordered_layout_ex")) return orc;
    CompiledScene cs;
    try {
        cs = compile_scene(*desc, true);
        build_ordered(cs, ordered_options_for(opt, tuning_snapshot()));
    } catch (const CompileError &e) {
        return fail(e.status, e.what());
    } catch (const std::exception &e) {
        return fail(RT_ERR_INVALID_ARGUMENT, std::string("rt_debug_ordered_layout: ") + e.what());
    }
    io->ordered = cs.ordered ? 1u : 0u;
    io->root = cs.ordered && cs.oseq[0].kind == OSEQ_TREE ? cs.oseq[0].a : 0u;
    io->n_steps = (int64_t)cs.oseq.size();
    if (io->steps) {
        if (io->cap_steps < io->n_steps) return fail(RT_ERR_INVALID_ARGUMENT, "rt_debug_ordered_layout: steps buffer too small");
        if (io->n_steps) memcpy(io->steps, cs.oseq.data(), cs.oseq.size() * sizeof(OSeq));
    }
    io->n_media = (int64_t)cs.media.size();
    if (io->media) {
        if (io->cap_media < io->n_media) return fail(RT_ERR_INVALID_ARGUMENT, "rt_debug_ordered_layout: media buffer too small");
        for (size_t i = 0; i < cs.media.size(); ++i) io->media[i] = cs.media[i].first_node;
    }
    io->stack_entries = cs.ordered_stack;
    io->n_nodes = (int64_t)cs.onodes.size(); io->n_spheres = (int64_t)cs.spheres.size();
    io->n_quads = (int64_t)cs.quads.size(); io->n_instances = (int64_t)cs.instances.size();
    if (io->nodes) {
        if (io->cap_nodes < io->n_nodes) return fail(RT_ERR_INVALID_ARGUMENT, "rt_debug_ordered_layout: nodes buffer too small");
        if (io->n_nodes) memcpy(io->nodes, cs.onodes.data(), cs.onodes.size() * sizeof(ONode));
    }
    if (io->spheres) {
        if (io->cap_spheres < io->n_spheres) return fail(RT_ERR_INVALID_ARGUMENT, "rt_debug_ordered_layout: spheres buffer too small");
        for (size_t i = 0; i < cs.spheres.size(); ++i) {
            const Sphere &sp = cs.spheres[i];
            double *o = io->spheres + i * 9;
            for (int k = 0; k < 3; ++k) { o[k] = sp.center[k]; o[4 + k] = sp.center_vec[k]; }
            o[3] = sp.radius; o[7] = (double)(sp.seq_moving >> 1); o[8] = (double)(sp.seq_moving & 1u);
        }
    }
    if (io->quads) {
        if (io->cap_quads < io->n_quads) return fail(RT_ERR_INVALID_ARGUMENT, "rt_debug_ordered_layout: quads buffer too small");
        for (size_t i = 0; i < cs.quads.size(); ++i) {
            const Quad &qd = cs.quads[i];
            double *o = io->quads + i * 10;
            for (int k = 0; k < 3; ++k) { o[k] = qd.q[k]; o[3 + k] = qd.u[k]; o[6 + k] = qd.v[k]; }
            o[9] = (double)qd.seq;
        }
    }
    if (io->instances) {
        if (io->cap_instances < io->n_instances) return fail(RT_ERR_INVALID_ARGUMENT, "rt_debug_ordered_layout: instances buffer too small");
        for (size_t i = 0; i < cs.instances.size(); ++i) {
            const Instance &in = cs.instances[i];
            double *o = io->instances + i * 8;
            for (int k = 0; k < 3; ++k) o[k] = in.offset[k];
            o[3] = in.sin_theta; o[4] = in.cos_theta; o[5] = (double)in.parent; o[6] = (double)in.flags; o[7] = (double)in.root;
        }
    }
    return RT_OK;
}

// Structure check of the wide layout (no device): walks every tree from its root and reports
//   out[0] records, out[1] primitives found in leaves, out[2] primitives of the scene's tables, out[3] stack entries a walk needs,
//   out[4] violations (a primitive in no leaf or in two, a child's box not inside its parent's slot, a reference out of range),
//   out[5] deepest chain of records
int rt_debug_wide_layout(const rt_scene_desc *desc, const rt_scene_options *options, uint64_t out[6]) {
    if (!desc || !out) return fail(RT_ERR_INVALID_ARGUMENT, "rt_debug_wide_layout: null argument");
    rt_scene_options opt;
    if (int orc = resolve_scene_options(options, opt, "rt_debug_wide_layout")) return orc;
    CompiledScene cs;
    try {
        cs = compile_scene(*desc, true);
        OrderedOptions oopt = ordered_options_for(opt, tuning_snapshot());
        oopt.wide = true;
        build_ordered(cs, oopt);
    } catch (const CompileError &e) {
        return fail(e.status, e.what());
    } catch (const std::exception &e) {
        return fail(RT_ERR_INVALID_ARGUMENT, std::string("rt_debug_wide_layout: ") + e.what());
    }
    for (int k = 0; k < 6; ++k) out[k] = 0;
    if (!cs.ordered || !cs.wide) return RT_OK;
    std::vector<uint32_t> seen_s(cs.spheres.size(), 0), seen_q(cs.quads.size(), 0), seen_r(cs.onodes4.size(), 0);
    uint64_t violations = 0, deepest = 0;
    struct Walk { uint32_t rec; uint64_t depth; };
    std::vector<Walk> todo;
    for (const OSeq &st : cs.oseq) {
        if (st.kind == OSEQ_TREE) todo.push_back({st.a, 1});
        else if (st.kind == OSEQ_MEDIUM) todo.push_back({st.b, 1});
    }
    for (const Instance &in : cs.instances) todo.push_back({in.root, 1});
    while (!todo.empty()) {
        const Walk w = todo.back();
        todo.pop_back();
        if (w.rec >= cs.onodes4.size()) { violations++; continue; }
        if (seen_r[w.rec]++) continue; // (an instance's root is reached from the table above and, as a child, never: each record once)
        deepest = std::max(deepest, w.depth);
        const ONode4 &nd = cs.onodes4[w.rec];
        for (int k = 0; k < 4; ++k) {
            const uint32_t kind = nd.c[k] >> OREF_KIND_SHIFT, index = nd.c[k] & OREF_INDEX_MASK, count = ((nd.c[k] >> OREF_COUNT_SHIFT) & OREF_COUNT_MASK) + 1u;
            if (kind == OK_EMPTY) { if (!(nd.b[k][0] > nd.b[k][1])) violations++; continue; } // an empty slot's box must admit no ray
            if (kind == OK_INNER) {
                if (index >= cs.onodes4.size()) { violations++; continue; }
                const ONode4 &ch = cs.onodes4[index];
                for (int q = 0; q < 4; ++q)
                    if ((ch.c[q] >> OREF_KIND_SHIFT) != OK_EMPTY)
                        for (int ax = 0; ax < 3; ++ax)
                            if (ch.b[q][2 * ax] < nd.b[k][2 * ax] || ch.b[q][2 * ax + 1] > nd.b[k][2 * ax + 1]) violations++;
                todo.push_back({index, w.depth + 1});
            } else if (kind == OK_SPHERES) {
                for (uint32_t i = 0; i < count; ++i) { if (index + i >= seen_s.size()) violations++; else seen_s[index + i]++; }
            } else if (kind == OK_QUADS) {
                for (uint32_t i = 0; i < count; ++i) { if (index + i >= seen_q.size()) violations++; else seen_q[index + i]++; }
            } else if (kind == OK_INSTANCE) {
                if (index >= cs.instances.size()) violations++;
            } else violations++;
        }
    }
    uint64_t found = 0;
    // (the boundary spheres of media solved in place are in no leaf: they sit behind the leaves' spheres, cs.media[].first_node)
    std::vector<bool> boundary(cs.spheres.size(), false);
    for (const OSeq &st : cs.oseq)
        if (st.kind == OSEQ_MEDIUM_SPHERE) boundary[cs.media[st.a].first_node] = true;
    for (size_t i = 0; i < seen_s.size(); ++i) { found += seen_s[i]; if (seen_s[i] != (boundary[i] ? 0u : 1u)) violations++; }
    for (size_t i = 0; i < seen_q.size(); ++i) { found += seen_q[i]; if (seen_q[i] != 1u) violations++; }
    out[0] = cs.onodes4.size(); out[1] = found; out[2] = cs.spheres.size() + cs.quads.size(); out[3] = cs.ordered_stack; out[4] = violations; out[5] = deepest;
    return RT_OK;
}

// the f64 bound of what a wide record's slots hold (rt_debug_wide_records): leaves from their primitives, inner records and
// instances from below, each record once
namespace {
struct WideBounds {
    const CompiledScene &cs;
    std::vector<Bound> slot;   // [record * 4 + k]
    std::vector<uint8_t> done; // per record
    explicit WideBounds(const CompiledScene &c) : cs(c), slot(c.onodes4.size() * 4), done(c.onodes4.size(), 0) {}
    Bound record(uint32_t rec) { // everything below the record
        Bound all;
        if (rec >= cs.onodes4.size()) return all;
        if (!done[rec]) {
            done[rec] = 1;
            const ONode4 &nd = cs.onodes4[rec];
            for (int k = 0; k < 4; ++k) {
                const uint32_t kind = nd.c[k] >> OREF_KIND_SHIFT, index = nd.c[k] & OREF_INDEX_MASK, count = ((nd.c[k] >> OREF_COUNT_SHIFT) & OREF_COUNT_MASK) + 1u;
                Bound b;
                if (kind == OK_INNER) b = record(index);
                else if (kind == OK_SPHERES) { for (uint32_t i = 0; i < count && index + i < cs.spheres.size(); ++i) b.add(sphere_bound(cs.spheres[index + i])); }
                else if (kind == OK_QUADS) { for (uint32_t i = 0; i < count && index + i < cs.quads.size(); ++i) b.add(quad_bound(cs.quads[index + i])); }
                else if (kind == OK_INSTANCE && index < cs.instances.size()) b = instance_bound(cs.instances[index], record(cs.instances[index].root));
                slot[(size_t)rec * 4 + k] = b;
            }
        }
        for (int k = 0; k < 4; ++k) all.add(slot[(size_t)rec * 4 + k]);
        return all;
    }
};
} // namespace

int rt_debug_wide_records(const rt_scene_desc *desc, const rt_scene_options *options, rt_debug_wide *io) {
    if (!desc || !io) return fail(RT_ERR_INVALID_ARGUMENT, "rt_debug_wide_records: null argument");
    rt_scene_options opt;
    if (int orc = resolve_scene_options(options, opt, "rt_debug_wide_records")) return orc;
    CompiledScene cs;
    if (int crc = compile_for_scene(*desc, opt, tuning_snapshot(), cs, "rt_debug_wide_records")) return crc;
    const bool wide = cs.ordered && cs.wide;
    const size_t n = wide ? cs.onodes4.size() : 0;
    io->wide = wide ? 1u : 0u;
    io->n_records = (int64_t)n;
    io->n_steps = cs.ordered ? (int64_t)cs.oseq.size() : 0;
    io->box_extent = ordered_box_extent(cs);
    io->table_bytes = (uint32_t)(n * 32);
    if ((io->boxes || io->refs || io->bounds || io->global_image || io->lds_image) && io->cap_records < io->n_records)
        return fail(RT_ERR_INVALID_ARGUMENT, "rt_debug_wide_records: record buffers too small");
    if (io->step_boxes && io->cap_steps < io->n_steps) return fail(RT_ERR_INVALID_ARGUMENT, "rt_debug_wide_records: steps buffer too small");
    if (io->step_boxes)
        for (int64_t i = 0; i < io->n_steps; ++i) memcpy(io->step_boxes + i * 6, cs.oseq[(size_t)i].box, 6 * sizeof(float));
    if (n == 0) return RT_OK;
    for (size_t i = 0; i < n; ++i) {
        if (io->boxes) memcpy(io->boxes + i * 24, cs.onodes4[i].b, 24 * sizeof(float));
        if (io->refs) memcpy(io->refs + i * 4, cs.onodes4[i].c, 4 * sizeof(uint32_t));
    }
    if (io->bounds) {
        WideBounds wb(cs);
        for (size_t i = 0; i < n; ++i) {
            wb.record((uint32_t)i);
            for (int k = 0; k < 4; ++k) {
                const Bound &b = wb.slot[i * 4 + k];
                for (int ax = 0; ax < 3; ++ax) { io->bounds[(i * 4 + k) * 6 + 2 * ax] = b.lo[ax]; io->bounds[(i * 4 + k) * 6 + 2 * ax + 1] = b.hi[ax]; }
            }
        }
    }
    if (io->global_image || io->lds_image) {
        const NodeTables img = pack_wide_records(cs.onodes4);
        if (io->global_image) memcpy(io->global_image, img.lines.data(), n * 256);
        if (io->lds_image) memcpy(io->lds_image, img.tables.data(), n * 208);
    }
    return RT_OK;
}

int rt_debug_scene_plan(const rt_scene_desc *desc, const rt_scene_options *options, rt_debug_plan *io) {
    if (!desc || !io) return fail(RT_ERR_INVALID_ARGUMENT, "rt_debug_scene_plan: null argument");
    rt_scene_options opt;
    if (int orc = resolve_scene_options(options, opt, "rt_debug_scene_plan")) return orc;
    ScenePlan plan;
    if (int prc = plan_scene(*desc, opt, tuning_snapshot(), plan, "rt_debug_scene_plan")) return prc;
    const Layout &l = plan.layout;
    io->features = l.features; io->parks_colours = l.parks_colours; io->has_instances = l.has_instances; io->ordered = l.ordered; io->wide = l.wide;
    io->o_root = l.o_root; io->n_oseq = l.n_oseq; io->o_stack = l.o_stack; io->n_nodes = l.n_nodes;
    io->o_start_stage = l.start.stage; io->o_start_prim = l.start.prim; io->o_start_end = l.start.end; io->o_start_rest = l.start.rest;
    io->o_start_slot = l.start.slot; io->o_start_direct = l.start.direct;
    io->box_extent = l.box_extent;
    io->lds_level = (uint32_t)l.lds.level; io->lds_off_node_b = l.lds.off_node_b; io->lds_off_spheres = l.lds.off_spheres;
    io->lds_off_quads = l.lds.off_quads; io->lds_off_qfilt = l.lds.off_qfilt;
    for (int k = 0; k < 4; ++k) io->lds_prefix_bytes[k] = l.lds.prefix_bytes[k];
    io->aux_bytes = l.aux.bytes;
    for (int k = 0; k < 5; ++k) io->aux_off[k] = l.aux.off[k];
    io->stats = plan.stats;
    for (int k = 0; k < 2; ++k) { // the two levels a scene may be launched at (rt_scene_options.use_lds = 0: level 0)
        const int lds = k ? l.lds.level : 0;
        rt_debug_plan_level &v = io->level[k];
        v.lds_level = (uint32_t)lds; v.features = kernel_features_for(l.features, lds, l.ordered); v.threads = (uint32_t)block_threads(l, lds);
        v.aux_in_lds = aux_in_lds(l, lds) ? 1u : 0u; v.world_in_lds = world_in_lds(l, lds) ? 1u : 0u;
        v.stack_off = l.lds.prefix_bytes[lds]; v.seq_off = (uint32_t)seq_offset(l, lds); v.aux_off = (uint32_t)aux_offset(l, lds);
        v.world_off = (uint32_t)world_offset(l, lds); v.prof_off = (uint32_t)prof_offset(l, lds);
        v.dynamic_lds_bytes = (uint32_t)dynamic_lds_bytes(l, lds, false); v.dynamic_lds_bytes_counted = (uint32_t)dynamic_lds_bytes(l, lds, true);
    }
    auto fnv1a = [](const void *data, size_t n) {
        uint64_t h = 0xcbf29ce484222325ull;
        for (size_t i = 0; i < n; ++i) { h ^= static_cast<const unsigned char *>(data)[i]; h *= 0x100000001b3ull; }
        return h;
    };
    int rc = RT_OK;
    auto give = [&](rt_debug_plan_bytes &out, const auto &v, uint8_t *buf = nullptr, int64_t cap = 0) {
        out.bytes = v.size() * sizeof(v[0]);
        out.digest = fnv1a(v.data(), out.bytes);
        if (buf && cap < (int64_t)out.bytes) rc = fail(RT_ERR_INVALID_ARGUMENT, "rt_debug_scene_plan: image buffer too small");
        else if (buf && out.bytes) memcpy(buf, v.data(), out.bytes);
    };
    const CompiledScene &cs = plan.cs;
    give(io->images[0], plan.oimage, io->oimage, io->cap_oimage); give(io->images[1], plan.lds_image, io->lds_image, io->cap_lds_image);
    give(io->images[2], plan.aux_image, io->aux_image, io->cap_aux_image); give(io->images[3], plan.mats, io->mats, io->cap_mats);
    give(io->tables[0], cs.nodes32); give(io->tables[1], cs.oseq); give(io->tables[2], cs.spheres); give(io->tables[3], cs.quads);
    give(io->tables[4], cs.instances, io->insts, io->cap_insts); give(io->tables[5], cs.media); give(io->tables[6], cs.textures);
    give(io->tables[7], cs.perlins); give(io->tables[8], cs.images); give(io->tables[9], cs.texels); give(io->tables[10], cs.srgb_lut);
    return rc;
}

int rt_debug_wide_visits(const rt_debug_wide_cases *io, int device) {
    if (!io || io->n <= 0 || !io->rays || !io->tmin || !io->tmax || !io->todo || !io->enter || !io->leave || !io->hit || !io->chosen ||
        !io->degenerate || !io->exact)
        return fail(RT_ERR_INVALID_ARGUMENT, "rt_debug_wide_visits: bad argument");
    const bool packed = io->boxes == nullptr;
    if (packed) {
        if (!io->global_image || !io->lds_image || !io->record || io->n_records <= 0) return fail(RT_ERR_INVALID_ARGUMENT, "rt_debug_wide_visits: neither boxes nor packed records");
        for (int64_t i = 0; i < io->n; ++i)
            if ((int64_t)io->record[i] >= io->n_records) return fail(RT_ERR_INVALID_ARGUMENT, "rt_debug_wide_visits: record index out of range");
    }
    if (rt_device_count() <= device || device < 0) return fail(RT_ERR_NO_DEVICE, "rt_debug_wide_visits: no such HIP device");
    HIP_TRY(hipSetDevice(device));
    const int64_t chunk_max = io->n < (1 << 18) ? io->n : (1 << 18); // cases per launch: 64 MiB of records
    const size_t image_row = io->lds != 0 ? 208 : 256;
    struct Buf { void *p = nullptr; size_t bytes; };
    Buf d_rays{nullptr, (size_t)chunk_max * 48}, d_boxes{nullptr, (size_t)chunk_max * 192}, d_tmin{nullptr, (size_t)chunk_max * 8}, d_tmax{nullptr, (size_t)chunk_max * 8},
        d_todo{nullptr, (size_t)chunk_max}, d_ext{nullptr, (size_t)chunk_max * 4}, d_image{nullptr, (size_t)chunk_max * image_row}, d_enter{nullptr, (size_t)chunk_max * 16},
        d_leave{nullptr, (size_t)chunk_max * 16}, d_hit{nullptr, (size_t)chunk_max}, d_chosen{nullptr, (size_t)chunk_max}, d_deg{nullptr, (size_t)chunk_max}, d_exact{nullptr, (size_t)chunk_max};
    Buf *all[] = {&d_rays, &d_boxes, &d_tmin, &d_tmax, &d_todo, &d_ext, &d_image, &d_enter, &d_leave, &d_hit, &d_chosen, &d_deg, &d_exact};
    int rc = RT_OK;
    for (Buf *b : all)
        if (rc == RT_OK && hipMalloc(&b->p, b->bytes) != hipSuccess) rc = fail(RT_ERR_OUT_OF_MEMORY, "rt_debug_wide_visits: hipMalloc failed");
    std::vector<ONode4> recs;
    std::vector<double> boxes64;
    std::vector<float> extents;
    std::vector<unsigned char> gathered;
    for (int64_t first = 0; first < io->n && rc == RT_OK; first += chunk_max) {
        const int64_t m = io->n - first < chunk_max ? io->n - first : chunk_max;
        recs.assign((size_t)m, ONode4{});
        boxes64.assign((size_t)m * 24, 0.0);
        extents.assign((size_t)m, 0.0f);
        const unsigned char *image = nullptr;
        NodeTables img;
        if (!packed) {
            for (int64_t i = 0; i < m; ++i) {
                const double *src = io->boxes + (first + i) * 24;
                ONode4 &nd = recs[(size_t)i];
                for (int k = 0; k < 4; ++k) {
                    const double *b = src + 6 * k;
                    double *b64 = &boxes64[(size_t)i * 24 + 6 * k];
                    const bool empty = b[0] > b[1] || b[2] > b[3] || b[4] > b[5];
                    for (int ax = 0; ax < 3; ++ax) {
                        b64[2 * ax] = empty ? (double)INFINITY : b[2 * ax];
                        b64[2 * ax + 1] = empty ? -(double)INFINITY : b[2 * ax + 1];
                        nd.b[k][2 * ax] = empty ? INFINITY : round_down(b[2 * ax]); // (rt_ordered.hpp set_child, widen)
                        nd.b[k][2 * ax + 1] = empty ? -INFINITY : round_up(b[2 * ax + 1]);
                    }
                    nd.c[k] = empty ? (OK_EMPTY << OREF_KIND_SHIFT) : (io->refs ? io->refs[(first + i) * 4 + k] : (OK_SPHERES << OREF_KIND_SHIFT));
                    if (!empty && (nd.c[k] >> OREF_KIND_SHIFT) >= OK_EMPTY) rc = fail(RT_ERR_INVALID_ARGUMENT, "rt_debug_wide_visits: an empty reference on a box");
                }
            }
            if (rc != RT_OK) break;
            img = pack_wide_records(recs);
            image = reinterpret_cast<const unsigned char *>(io->lds != 0 ? img.tables.data() : img.lines.data());
        } else {
            // the rows of the caller's image that the cases visit, gathered byte for byte into an image of m records
            gathered.assign((size_t)m * image_row, 0);
            const size_t src_table = (size_t)io->n_records * 32, dst_table = (size_t)m * 32;
            for (int64_t i = 0; i < m; ++i) {
                const size_t rec = io->record[first + i];
                if (io->lds != 0) {
                    for (size_t q = 0; q < 6; ++q) memcpy(&gathered[q * dst_table + (size_t)i * 32], io->lds_image + q * src_table + rec * 32, 32);
                    memcpy(&gathered[6 * dst_table + (size_t)i * 16], io->lds_image + 6 * src_table + rec * 16, 16);
                } else {
                    memcpy(&gathered[(size_t)i * 256], io->global_image + rec * 256, 256);
                }
                // the boxes back out of the record's "+" tables (enter through lo, leave through hi), for the exact test and the extent
                const float *line = reinterpret_cast<const float *>(io->global_image + rec * 256);
                for (int k = 0; k < 4; ++k)
                    for (int ax = 0; ax < 3; ++ax) {
                        recs[(size_t)i].b[k][2 * ax] = line[16 * ax + k];
                        recs[(size_t)i].b[k][2 * ax + 1] = line[16 * ax + 4 + k];
                        boxes64[(size_t)i * 24 + 6 * k + 2 * ax] = (double)line[16 * ax + k];
                        boxes64[(size_t)i * 24 + 6 * k + 2 * ax + 1] = (double)line[16 * ax + 4 + k];
                    }
                memcpy(recs[(size_t)i].c, io->global_image + rec * 256 + 192, 16);
            }
            image = gathered.data();
        }
        for (int64_t i = 0; i < m; ++i)
            for (int k = 0; k < 4; ++k)
                if ((recs[(size_t)i].c[k] >> OREF_KIND_SHIFT) != OK_EMPTY)
                    for (int q = 0; q < 6; ++q) extents[(size_t)i] = std::fmax(extents[(size_t)i], std::fabs(recs[(size_t)i].b[k][q]));
        const bool up = hipMemcpy(d_rays.p, io->rays + first * 6, (size_t)m * 48, hipMemcpyHostToDevice) == hipSuccess &&
                        hipMemcpy(d_boxes.p, boxes64.data(), (size_t)m * 192, hipMemcpyHostToDevice) == hipSuccess &&
                        hipMemcpy(d_tmin.p, io->tmin + first, (size_t)m * 8, hipMemcpyHostToDevice) == hipSuccess &&
                        hipMemcpy(d_tmax.p, io->tmax + first, (size_t)m * 8, hipMemcpyHostToDevice) == hipSuccess &&
                        hipMemcpy(d_todo.p, io->todo + first, (size_t)m, hipMemcpyHostToDevice) == hipSuccess &&
                        hipMemcpy(d_ext.p, extents.data(), (size_t)m * 4, hipMemcpyHostToDevice) == hipSuccess &&
                        hipMemcpy(d_image.p, image, (size_t)m * image_row, hipMemcpyHostToDevice) == hipSuccess;
        if (!up) { rc = fail(RT_ERR_HIP, "rt_debug_wide_visits: upload failed"); break; }
        DebugWideArgs a{};
        a.n = m;
        a.rays = (const double *)d_rays.p; a.boxes = (const double *)d_boxes.p; a.tmin = (const double *)d_tmin.p; a.tmax = (const double *)d_tmax.p;
        a.todo = (const uint8_t *)d_todo.p;
        a.extents = io->extent > 0.0f ? nullptr : (const float *)d_ext.p;
        a.extent = io->extent;
        a.image = (const uint4 *)d_image.p;
        a.enter = (float *)d_enter.p; a.leave = (float *)d_leave.p;
        a.hit = (uint8_t *)d_hit.p; a.degenerate = (uint8_t *)d_deg.p; a.exact = (uint8_t *)d_exact.p; a.chosen = (int8_t *)d_chosen.p;
        launch_debug_wide(a, io->lds);
        const bool down = hipMemcpy(io->enter + first * 4, d_enter.p, (size_t)m * 16, hipMemcpyDeviceToHost) == hipSuccess &&
                          hipMemcpy(io->leave + first * 4, d_leave.p, (size_t)m * 16, hipMemcpyDeviceToHost) == hipSuccess &&
                          hipMemcpy(io->hit + first, d_hit.p, (size_t)m, hipMemcpyDeviceToHost) == hipSuccess &&
                          hipMemcpy(io->chosen + first, d_chosen.p, (size_t)m, hipMemcpyDeviceToHost) == hipSuccess &&
                          hipMemcpy(io->degenerate + first, d_deg.p, (size_t)m, hipMemcpyDeviceToHost) == hipSuccess &&
                          hipMemcpy(io->exact + first, d_exact.p, (size_t)m, hipMemcpyDeviceToHost) == hipSuccess;
        if (!down) { rc = fail(RT_ERR_HIP, std::string("rt_debug_wide_visits: ") + hipGetErrorString(hipGetLastError())); break; }
    }
    for (Buf *b : all) (void)hipFree(b->p);
    return rc;
}

int rt_debug_compiled_nodes(const rt_scene_desc *desc, int32_t refit, rt_debug_node *out_nodes, int64_t capacity, int64_t *out_count) {
    if (!desc || !out_count) return fail(RT_ERR_INVALID_ARGUMENT, "rt_debug_compiled_nodes: null argument");
    CompiledScene cs;
    try {
        cs = compile_scene(*desc, refit != 0);
    } catch (const CompileError &e) {
        return fail(e.status, e.what());
    } catch (const std::exception &e) {
        return fail(RT_ERR_INVALID_ARGUMENT, std::string("rt_debug_compiled_nodes: ") + e.what());
    }
    *out_count = (int64_t)cs.nodes.size();
    if (!out_nodes) return RT_OK;
    if ((int64_t)cs.nodes.size() > capacity) return fail(RT_ERR_INVALID_ARGUMENT, "rt_debug_compiled_nodes: buffer too small");
    for (size_t i = 0; i < cs.nodes.size(); ++i) {
        const Node &n = cs.nodes[i];
        const Node32 &m = cs.nodes32[i];
        rt_debug_node &o = out_nodes[i];
        for (int k = 0; k < 3; ++k) { o.lo[k] = n.lo[k]; o.hi[k] = n.hi[k]; }
        o.lo32[0] = m.bx[0]; o.hi32[0] = m.bx[1]; o.lo32[1] = m.by[0]; o.hi32[1] = m.by[1]; o.lo32[2] = m.bz[0]; o.hi32[2] = m.bz[1];
        o.skip = n.skip; o.kind = n.kind & NODE_KIND_MASK; o.no_bbox = (n.kind & NODE_NO_BBOX) ? 1u : 0u; o.a = n.a; o.b = n.b;
        o.prim_lo[0] = o.prim_lo[1] = o.prim_lo[2] = INFINITY;
        o.prim_hi[0] = o.prim_hi[1] = o.prim_hi[2] = -INFINITY;
        // bound of the record's own primitives (leaves), in the frame the record lives in
        auto grow = [&](double x, double y, double z) {
            const double p[3] = {x, y, z};
            for (int k = 0; k < 3; ++k) { o.prim_lo[k] = std::fmin(o.prim_lo[k], p[k]); o.prim_hi[k] = std::fmax(o.prim_hi[k], p[k]); }
        };
        if (o.kind == NK_SPHERES || o.kind == NK_MEDIUM_SPHERE) {
            const uint32_t first = o.kind == NK_SPHERES ? n.a : cs.media[n.a].first_node, count = o.kind == NK_SPHERES ? n.b : 1u;
            for (uint32_t q = first; q < first + count; ++q) {
                const Sphere &sp = cs.spheres[q];
                for (int e = 0; e < ((sp.seq_moving & 1u) ? 2 : 1); ++e) {
                    const double c[3] = {sp.center[0] + e * sp.center_vec[0], sp.center[1] + e * sp.center_vec[1], sp.center[2] + e * sp.center_vec[2]};
                    grow(c[0] - sp.radius, c[1] - sp.radius, c[2] - sp.radius);
                    grow(c[0] + sp.radius, c[1] + sp.radius, c[2] + sp.radius);
                }
            }
        } else if (o.kind == NK_QUADS) {
            for (uint32_t q = n.a; q < n.a + n.b; ++q) {
                const Quad &qd = cs.quads[q];
                for (int i2 = 0; i2 < 2; ++i2)
                    for (int j2 = 0; j2 < 2; ++j2)
                        grow(qd.q[0] + i2 * qd.u[0] + j2 * qd.v[0], qd.q[1] + i2 * qd.u[1] + j2 * qd.v[1], qd.q[2] + i2 * qd.u[2] + j2 * qd.v[2]);
            }
        }
    }
    return RT_OK;
}

int rt_debug_last_launch(uint32_t out[4]) {
    if (!out) return fail(RT_ERR_INVALID_ARGUMENT, "rt_debug_last_launch: null argument");
    for (int k = 0; k < 4; ++k) out[k] = g_last_launch[k];
    return RT_OK;
}

int rt_debug_last_kernel(uint32_t out[8]) {
    if (!out) return fail(RT_ERR_INVALID_ARGUMENT, "rt_debug_last_kernel: null argument");
    for (int k = 0; k < 8; ++k) out[k] = g_last_kernel[k];
    return RT_OK;
}

int rt_debug_last_start(uint32_t out[4]) {
    if (!out) return fail(RT_ERR_INVALID_ARGUMENT, "rt_debug_last_start: null argument");
    for (int k = 0; k < 4; ++k) out[k] = g_last_start[k];
    return RT_OK;
}

int rt_debug_adaptive_step(int64_t n_list,const uint32_t *list, int64_t n_pixels, const double *sum, const double *sum_sq, int32_t n,
                           int32_t last, double rel_threshold, double abs_threshold, int32_t *spp, uint32_t *list_out, uint32_t *out_count,
                           int device) {
    if (!list || !sum || !sum_sq || !spp || !list_out || !out_count) return fail(RT_ERR_INVALID_ARGUMENT, "rt_debug_adaptive_step: null argument");
    if (n_list <= 0 || n_list % 64 != 0 || n_list > ((int64_t)1 << 27))
        return fail(RT_ERR_INVALID_ARGUMENT, "rt_debug_adaptive_step: n_list must be a positive multiple of 64, at most 2^27");
    if (n_pixels <= 0 || n_pixels >= ((int64_t)1 << 27)) return fail(RT_ERR_INVALID_ARGUMENT, "rt_debug_adaptive_step: n_pixels must be positive and below 2^27");
    if (rt_device_count() <= device || device < 0) return fail(RT_ERR_NO_DEVICE, "rt_debug_adaptive_step: no such HIP device");
    HIP_TRY(hipSetDevice(device));
    // the step's scratch as render_adaptive lays it out; behind it the frame's sums, squared sums and sample counts
    const size_t step_bytes = adaptive_scratch_layout((uint32_t)n_list, nullptr, nullptr, nullptr);
    const size_t sum_bytes = (size_t)n_pixels * 3u * sizeof(double), spp_bytes = (size_t)n_pixels * sizeof(int32_t), list_bytes = (size_t)n_list * 4u;
    char *buf = nullptr;
    if (hipMalloc((void **)&buf, step_bytes + 2u * sum_bytes + spp_bytes) != hipSuccess) {
        (void)hipGetLastError();
        return fail(RT_ERR_OUT_OF_MEMORY, "rt_debug_adaptive_step: hipMalloc failed");
    }
    uint32_t *d_list[2];
    AdaptiveScratch x;
    adaptive_scratch_layout((uint32_t)n_list, buf, d_list, &x);
    double *d_sum = (double *)(buf + step_bytes), *d_sq = (double *)(buf + step_bytes + sum_bytes);
    int32_t *d_spp = (int32_t *)(buf + step_bytes + 2u * sum_bytes);
    int rc = RT_OK;
    do {
        if (hipMemcpy(d_list[0], list, list_bytes, hipMemcpyHostToDevice) != hipSuccess ||
            hipMemcpy(d_list[1], list_out, list_bytes, hipMemcpyHostToDevice) != hipSuccess ||
            hipMemcpy(d_sum, sum, sum_bytes, hipMemcpyHostToDevice) != hipSuccess ||
            hipMemcpy(d_sq, sum_sq, sum_bytes, hipMemcpyHostToDevice) != hipSuccess ||
            hipMemcpy(d_spp, spp, spp_bytes, hipMemcpyHostToDevice) != hipSuccess) { rc = fail(RT_ERR_HIP, "rt_debug_adaptive_step: upload failed"); break; }
        launch_adaptive_step(d_list[0], (uint32_t)n_list, (uint32_t)n_pixels, d_sum, d_sq, n, last, rel_threshold, abs_threshold, d_spp, d_list[1], x, nullptr);
        hipError_t e = hipGetLastError();
        if (e == hipSuccess) e = hipMemcpy(out_count, x.count, sizeof(uint32_t), hipMemcpyDeviceToHost);
        if (e == hipSuccess) e = hipMemcpy(list_out, d_list[1], list_bytes, hipMemcpyDeviceToHost);
        if (e == hipSuccess) e = hipMemcpy(spp, d_spp, spp_bytes, hipMemcpyDeviceToHost);
        if (e != hipSuccess) { rc = fail(RT_ERR_HIP, std::string("rt_debug_adaptive_step: ") + hipGetErrorString(e)); break; }
    } while (0);
    (void)hipFree(buf);
    return rc;
}

int rt_debug_stage_profile(uint64_t out[36]) {
    if (!out) return fail(RT_ERR_INVALID_ARGUMENT, "rt_debug_stage_profile: null argument");
    std::lock_guard<std::mutex> lock(g_stage_profile_mu);
    for (uint32_t q = 0; q < PROF_SLOTS * 3u; ++q) out[q] = g_stage_profile[q];
    return RT_OK;
}

int rt_debug_visit_stats(uint64_t out[12]) {
    if (!out) return fail(RT_ERR_INVALID_ARGUMENT, "rt_debug_visit_stats: null argument");
    static_assert(VISIT_STATS == 12, "rt_amd_debug.h documents 12 words");
    std::lock_guard<std::mutex> lock(g_stage_profile_mu);
    for (uint32_t q = 0; q < VISIT_STATS; ++q) out[q] = g_visit_stats[q];
    return RT_OK;
}

int rt_debug_box_tests(int64_t n, const double *rays, const double *boxes, double tmin, double tmax, uint8_t *out_exact_hit,
                       uint8_t *out_f32_hit, int device) {
    if (n <= 0 || !rays || !boxes || !out_exact_hit || !out_f32_hit) return fail(RT_ERR_INVALID_ARGUMENT, "rt_debug_box_tests: bad argument");
    if (rt_device_count() <= device || device < 0) return fail(RT_ERR_NO_DEVICE, "rt_debug_box_tests: no such HIP device");
    HIP_TRY(hipSetDevice(device));
    double *dr = nullptr, *db = nullptr;
    uint8_t *de = nullptr, *df = nullptr;
    const size_t bytes = (size_t)n * 6 * sizeof(double);
    int rc = RT_OK;
    do {
        if (hipMalloc((void **)&dr, bytes) != hipSuccess || hipMalloc((void **)&db, bytes) != hipSuccess ||
            hipMalloc((void **)&de, (size_t)n) != hipSuccess || hipMalloc((void **)&df, (size_t)n) != hipSuccess) {
            rc = fail(RT_ERR_OUT_OF_MEMORY, "rt_debug_box_tests: hipMalloc failed"); break;
        }
        if (hipMemcpy(dr, rays, bytes, hipMemcpyHostToDevice) != hipSuccess || hipMemcpy(db, boxes, bytes, hipMemcpyHostToDevice) != hipSuccess) {
            rc = fail(RT_ERR_HIP, "rt_debug_box_tests: upload failed"); break;
        }
        launch_debug_box(n, dr, db, tmin, tmax, de, df);
        if (hipMemcpy(out_exact_hit, de, (size_t)n, hipMemcpyDeviceToHost) != hipSuccess ||
            hipMemcpy(out_f32_hit, df, (size_t)n, hipMemcpyDeviceToHost) != hipSuccess) {
            rc = fail(RT_ERR_HIP, "rt_debug_box_tests: download failed"); break;
        }
    } while (0);
    (void)hipFree(dr); (void)hipFree(db); (void)hipFree(de); (void)hipFree(df);
    return rc;
}

int rt_debug_quad_filter_tests(int64_t n, const double *rays, const double *quads, double tmin, double tmax, uint8_t *out_exact_hit,
                               uint8_t *out_keep, int device) {
    if (n <= 0 || !rays || !quads || !out_exact_hit || !out_keep) return fail(RT_ERR_INVALID_ARGUMENT, "rt_debug_quad_filter_tests: bad argument");
    if (rt_device_count() <= device || device < 0) return fail(RT_ERR_NO_DEVICE, "rt_debug_quad_filter_tests: no such HIP device");
    HIP_TRY(hipSetDevice(device));
    std::vector<Quad> hq((size_t)n);
    std::vector<QFiltPair> hf((size_t)n);
    for (int64_t i = 0; i < n; ++i) { // Quad::new (src/quad.rs:24-27)
        const double *s = quads + i * 9;
        Quad &q = hq[(size_t)i];
        memset(&q, 0, sizeof q);
        for (int k = 0; k < 3; ++k) { q.q[k] = s[k]; q.u[k] = s[3 + k]; q.v[k] = s[6 + k]; }
        const double nn[3] = {q.u[1] * q.v[2] - q.u[2] * q.v[1], q.u[2] * q.v[0] - q.u[0] * q.v[2], q.u[0] * q.v[1] - q.u[1] * q.v[0]};
        const double n2 = nn[0] * nn[0] + nn[1] * nn[1] + nn[2] * nn[2];
        const double rl = 1.0 / std::sqrt(n2), rn = 1.0 / n2;
        for (int k = 0; k < 3; ++k) { q.normal[k] = nn[k] * rl; q.w[k] = nn[k] * rn; }
        q.d = q.normal[0] * q.q[0] + q.normal[1] * q.q[1] + q.normal[2] * q.q[2];
        memset(&hf[(size_t)i], 0, sizeof(QFiltPair));
    }
    for (int64_t i = 0; i < n; ++i) { // (the quad sits in both slots of its record: the pair's bounds are its own)
        qfilt_fill(hq[(size_t)i], hf[(size_t)i], 0);
        qfilt_fill(hq[(size_t)i], hf[(size_t)i], 1);
    }
    double *dr = nullptr;
    Quad *dq = nullptr;
    QFiltPair *df = nullptr;
    uint8_t *de = nullptr, *dk = nullptr;
    int rc = RT_OK;
    do {
        if (hipMalloc((void **)&dr, (size_t)n * 6 * sizeof(double)) != hipSuccess || hipMalloc((void **)&dq, (size_t)n * sizeof(Quad)) != hipSuccess ||
            hipMalloc((void **)&df, (size_t)n * sizeof(QFiltPair)) != hipSuccess || hipMalloc((void **)&de, (size_t)n) != hipSuccess ||
            hipMalloc((void **)&dk, (size_t)n) != hipSuccess) { rc = fail(RT_ERR_OUT_OF_MEMORY, "rt_debug_quad_filter_tests: hipMalloc failed"); break; }
        if (hipMemcpy(dr, rays, (size_t)n * 6 * sizeof(double), hipMemcpyHostToDevice) != hipSuccess ||
            hipMemcpy(dq, hq.data(), (size_t)n * sizeof(Quad), hipMemcpyHostToDevice) != hipSuccess ||
            hipMemcpy(df, hf.data(), (size_t)n * sizeof(QFiltPair), hipMemcpyHostToDevice) != hipSuccess) { rc = fail(RT_ERR_HIP, "rt_debug_quad_filter_tests: upload failed"); break; }
        launch_debug_quad(n, dr, dq, df, tmin, tmax, de, dk);
        if (hipMemcpy(out_exact_hit, de, (size_t)n, hipMemcpyDeviceToHost) != hipSuccess || hipMemcpy(out_keep, dk, (size_t)n, hipMemcpyDeviceToHost) != hipSuccess) {
            rc = fail(RT_ERR_HIP, "rt_debug_quad_filter_tests: download failed"); break;
        }
    } while (0);
    (void)hipFree(dr); (void)hipFree(dq); (void)hipFree(df); (void)hipFree(de); (void)hipFree(dk);
    return rc;
}

int rt_debug_eval(int32_t op, int64_t n, const double *a, const double *b, double *out, int device) {
    if (n <= 0 || !a || !out) return fail(RT_ERR_INVALID_ARGUMENT, "rt_debug_eval: bad argument");
    if (rt_device_count() <= device || device < 0) return fail(RT_ERR_NO_DEVICE, "rt_debug_eval: no such HIP device");
    HIP_TRY(hipSetDevice(device));
    double *da = nullptr, *db = nullptr, *dout = nullptr;
    const size_t bytes = (size_t)n * sizeof(double);
    int rc = RT_OK;
    do {
        if (hipMalloc((void **)&da, bytes) != hipSuccess || hipMalloc((void **)&dout, bytes) != hipSuccess ||
            (b && hipMalloc((void **)&db, bytes) != hipSuccess)) { rc = fail(RT_ERR_OUT_OF_MEMORY, "rt_debug_eval: hipMalloc failed"); break; }
        if (hipMemcpy(da, a, bytes, hipMemcpyHostToDevice) != hipSuccess ||
            (b && hipMemcpy(db, b, bytes, hipMemcpyHostToDevice) != hipSuccess)) { rc = fail(RT_ERR_HIP, "rt_debug_eval: upload failed"); break; }
        launch_debug_eval(op, n, da, db, dout);
        hipError_t e = hipMemcpy(out, dout, bytes, hipMemcpyDeviceToHost);
        if (e != hipSuccess) { rc = fail(RT_ERR_HIP, std::string("rt_debug_eval: ") + hipGetErrorString(e)); break; }
    } while (0);
    (void)hipFree(da); (void)hipFree(db); (void)hipFree(dout);
    return rc;
}

} // extern "C"
