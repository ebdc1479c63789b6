// rt_scene_plan.cpp — the scene plan (rt_scene_plan.hpp): compile, then one named step per decision.  Host code only, no hip* call.
#include "rt_scene_plan.hpp"
#include "rt_qfilt.hpp"

#include <cmath>
#include <cstdlib>
#include <cstring>
#include <new>

namespace rtapi {

thread_local std::string g_last_error;

int fail(int status, const std::string &msg) {
    g_last_error = msg;
    return status;
}

Tuning::Tuning() {
    auto env = [](const char *name, int &v) { if (const char *e = getenv(name)) v = atoi(e); };
    env("RT_TH_PRIM", forced[0]); env("RT_TH_OTHER", forced[1]); env("RT_TH_SHADE", forced[2]); env("RT_TH_BOX", forced[3]); env("RT_TH_NEW", forced[4]);
    env("RT_USE_LDS", use_lds); env("RT_REFIT", refit); env("RT_ORDERED", ordered); env("RT_JOBS_PER_GRAB", jobs_per_grab); env("RT_GRAB_TAPER", grab_taper); env("RT_DEFER", defer); env("RT_START_SHORTCUT", start_shortcut); env("RT_START_INLINE", start_inline); env("RT_SEQ_LOOKAHEAD", seq_lookahead); env("RT_SLOW_MIN", slow_min); env("RT_SLOW_AGE", slow_age); env("RT_OVERLAP", overlap);
    env("RT_WIDE", wide); env("RT_WIDE_SETASIDE", wide_setaside); env("RT_QUAD_FILTER", quad_filter); env("RT_MEDIUM_FIRST", medium_first);
    if (const char *e = getenv("RT_SAH_LEAF")) ordered_options.leaf_max = (uint32_t)atoi(e);
    if (const char *e = getenv("RT_FLAT_MAX")) ordered_options.flat_max = (uint32_t)atoi(e);
    if (const char *e = getenv("RT_SAH_SPHERE")) ordered_options.cost_sphere = atof(e);
    if (const char *e = getenv("RT_SAH_QUAD")) ordered_options.cost_quad = atof(e);
    if (const char *e = getenv("RT_SAH_INSTANCE")) ordered_options.cost_instance = atof(e);
    if (const char *e = getenv("RT_SAMPLE_BUFFER_MB")) sample_buffer_bytes = (size_t)strtoull(e, nullptr, 10) << 20;
}

OrderedOptions ordered_options_for(const rt_scene_options &opt, const Tuning &tn) {
    OrderedOptions oopt = tn.ordered_options;
    if (opt.leaf_max > 0) oopt.leaf_max = (uint32_t)opt.leaf_max < OREF_MAX_LEAF ? (uint32_t)opt.leaf_max : OREF_MAX_LEAF;
    if (opt.flat_max >= 0) oopt.flat_max = (uint32_t)opt.flat_max;
    return oopt;
}

// Which walk for this scene?  Measured on MI355X at the in-code cameras (tools/scene_speed.py, profiles/r02_scene_speed.txt), own trees
// vs reference order, Msamples/s: random_balls 4416 / 2128, two_spheres 8739 / 7281, earth 22557 / 22523 (one primitive: a tree and a
// stack are pure overhead), two_perlin_spheres 4821 / 3288, quads 12860 / 12612, simple_light 5845 / 4894, cornell_box 3224 / 2102,
// cornell_smoke 1261 / 966 (a tie until its frames' primitives went into flat leaves, rt_ordered.hpp flat_max), final_scene 983 / 643.
static bool ordered_walk_pays(const CompiledScene &cs) {
    return cs.spheres.size() + cs.quads.size() > 1;
}

int compile_for_scene(const rt_scene_desc &desc, const rt_scene_options &opt, const Tuning &tn, CompiledScene &cs, const char *who) {
    const int walk = opt.walk != RT_WALK_DEFAULT ? opt.walk : tn.ordered;
    const bool refit = opt.refit >= 0 ? opt.refit != 0 : tn.refit != 0;
    OrderedOptions oopt = ordered_options_for(opt, tn);
    const int want_wide = opt.wide >= 0 ? opt.wide : tn.wide; // (-1: where it measured faster, below)
    try {
        cs = compile_scene(desc, refit);
        // Four children per record where the trees are big enough for the halved number of visits to pay for the dearer visit
        // (MI355X, Msamples/s two / four children: random-spheres 5428 / 5437, final_scene 1049 / 1088; Cornell's 4 records: 2438 / 2345)
        oopt.wide = want_wide >= 0 ? want_wide != 0 : cs.spheres.size() + cs.quads.size() >= 64;
        if (walk == RT_WALK_OWN_TREES || (walk == RT_WALK_AUTO && ordered_walk_pays(cs))) build_ordered(cs, oopt);
    } catch (const CompileError &e) {
        return fail(e.status, e.what());
    } catch (const std::exception &e) {
        return fail(RT_ERR_INVALID_ARGUMENT, std::string(who) + ": " + e.what());
    }
    return RT_OK;
}

// The largest |coordinate| of any box an ordered walk tests (box_pair_f32's and box_quad_f32's B): the children's boxes of the binary
// records — a wide record's slots are copies of those (rt_ordered.hpp widen) — and the boxes of the world's sequence.
float ordered_box_extent(const CompiledScene &cs) {
    float extent = 0.0f;
    for (const ONode &nd : cs.onodes)
        for (int k = 0; k < 6; ++k) {
            if ((nd.c[0] >> OREF_KIND_SHIFT) != OK_EMPTY) extent = std::fmax(extent, std::fabs(nd.b0[k]));
            if ((nd.c[1] >> OREF_KIND_SHIFT) != OK_EMPTY) extent = std::fmax(extent, std::fabs(nd.b1[k]));
        }
    for (const OSeq &st : cs.oseq)
        for (int k = 0; k < 6; ++k) extent = std::fmax(extent, std::fabs(st.box[k]));
    return extent;
}

NodeTables pack_wide_records(const std::vector<ONode4> &recs) {
    const size_t n = recs.size(), off_b = n * 32;
    NodeTables img;
    img.table_bytes = off_b;
    img.records = n;
    img.tables.resize(n * 13); // 6 x 32 + 16 bytes per record
    img.lines.resize(n * 16);
    unsigned char *base = reinterpret_cast<unsigned char *>(img.tables.data());
    for (size_t i = 0; i < n; ++i) {
        const ONode4 &nd = recs[i];
        for (int ax = 0; ax < 3; ++ax) {
            float plus[8], minus[8];
            for (int k = 0; k < 4; ++k) {
                plus[k] = nd.b[k][2 * ax]; plus[4 + k] = nd.b[k][2 * ax + 1];   // enter through lo, leave through hi
                minus[k] = nd.b[k][2 * ax + 1]; minus[4 + k] = nd.b[k][2 * ax];
            }
            memcpy(base + (size_t)(2 * ax) * off_b + i * 32, plus, 32);
            memcpy(base + (size_t)(2 * ax + 1) * off_b + i * 32, minus, 32);
        }
        memcpy(base + 6 * off_b + i * 16, nd.c, 16);
    }
    unsigned char *dst = reinterpret_cast<unsigned char *>(img.lines.data());
    for (size_t i = 0; i < n; ++i) {
        for (size_t q = 0; q < 6; ++q) memcpy(dst + i * 256 + q * 32, base + q * off_b + i * 32, 32);
        memcpy(dst + i * 256 + 192, base + 6 * off_b + i * 16, 16);
    }
    return img;
}

namespace {

bool texture_needs_uv(const std::vector<rt_texture> &texs, int32_t t, int depth = 0) {
    if (t < 0 || depth > 16) return false;
    const rt_texture &x = texs[(size_t)t];
    if (x.kind == RT_TEXTURE_IMAGE) return true;
    if (x.kind == RT_TEXTURE_CHECKER) return texture_needs_uv(texs, x.even, depth + 1) || texture_needs_uv(texs, x.odd, depth + 1);
    return false;
}

// Perlin turbulence anywhere under texture t (seven noise evaluations per lookup: by far the dearest thing a hit can ask for)
bool texture_has_noise(const std::vector<rt_texture> &texs, int32_t t, int depth = 0) {
    if (t < 0 || depth > 16) return false;
    const rt_texture &x = texs[(size_t)t];
    if (x.kind == RT_TEXTURE_NOISE) return true;
    if (x.kind == RT_TEXTURE_CHECKER) return texture_has_noise(texs, x.even, depth + 1) || texture_has_noise(texs, x.odd, depth + 1);
    return false;
}

// Step 1, features: which kernel class the scene gets and how its queries walk — the first block of the Layout, complete
Layout walk_layout(const CompiledScene &cs) {
    Layout l;
    l.has_instances = !cs.instances.empty();
    l.features = (cs.spheres.empty() ? 0u : F_SPHERES) | (cs.quads.empty() ? 0u : F_QUADS) | (cs.instances.empty() ? 0u : F_FRAMES) |
                 (cs.media.empty() ? 0u : F_MEDIA);
    for (const auto &t : cs.textures)
        if (t.kind != RT_TEXTURE_SOLID) l.features |= F_TEXTURES;
    // attenuations are parked as material indices unless the colour is a texture's value, or the indices do not fit 16 bits: such a
    // scene is rendered by the kernels that can park colours, i.e. those with textures
    if (cs.materials.size() >= 0xffffu) l.features |= F_TEXTURES;
    l.parks_colours = (l.features & F_TEXTURES) != 0;
    l.ordered = cs.ordered;
    l.wide = cs.ordered && cs.wide;
    // a walk starts in the first step's tree; a sequence that starts with a medium goes through ST_OTHER first
    l.o_root = cs.ordered && cs.oseq[0].kind == OSEQ_TREE ? cs.oseq[0].a : 0xfffffffeu;
    l.n_oseq = (uint32_t)cs.oseq.size();
    l.o_stack = cs.ordered_stack;
    l.n_nodes = (uint32_t)cs.nodes.size();
    l.box_extent = ordered_box_extent(cs);
    return l;
}

// Step 2, start shortcut.  random-spheres' ground sphere (r = 1000) spans the scene, so the sweep puts it directly under the root and every
// ray's origin lies inside its box — the walk visits the root, finds that leaf "nearest", tests the sphere, comes back for the other
// child; a frame of a few primitives keeps them in one leaf under its root (rt_ordered.hpp flat_max: Cornell's walls).  When the root
// has such a child (a leaf whose box has at least half the area of the root's), a query starts in the leaf's primitive stage with the
// other child already set aside: the same tests, minus the visit of the root record, and the lanes that start together stay together.
ScenePlan::Start start_shortcut(const CompiledScene &cs, bool wide, uint32_t o_root) {
    ScenePlan::Start st;
    if (!(cs.ordered && cs.media.empty() && cs.oseq.size() == 1 && cs.oseq[0].kind == OSEQ_TREE)) return st;
    auto half_area = [](const float *b) { const double x = (double)b[1] - b[0], y = (double)b[3] - b[2], z = (double)b[5] - b[4]; return x * y + y * z + z * x; };
    // the root's children: (box, reference) in slot order — two of a binary record, up to four of a wide one
    std::vector<std::pair<const float *, uint32_t>> kids;
    if (wide) {
        const ONode4 &root = cs.onodes4[o_root];
        for (int k = 0; k < 4; ++k) kids.emplace_back(root.b[k], root.c[k]);
    } else {
        const ONode &root = cs.onodes[o_root];
        kids.emplace_back(root.b0, root.c[0]);
        kids.emplace_back(root.b1, root.c[1]);
    }
    float all[6] = {INFINITY, -INFINITY, INFINITY, -INFINITY, INFINITY, -INFINITY};
    for (const auto &kid : kids)
        if ((kid.second >> OREF_KIND_SHIFT) != OK_EMPTY)
            for (int k = 0; k < 6; k += 2) { all[k] = std::fmin(all[k], kid.first[k]); all[k + 1] = std::fmax(all[k + 1], kid.first[k + 1]); }
    for (uint32_t slot = 0; slot < kids.size(); ++slot) {
        const uint32_t ref = kids[slot].second, kind = ref >> OREF_KIND_SHIFT;
        if ((kind == OK_SPHERES || kind == OK_QUADS) && half_area(kids[slot].first) >= 0.5 * half_area(all)) {
            st.stage = kind; // (OrderedKind SPHERES / QUADS = Stage ST_SPHERE / ST_QUAD)
            st.prim = ref & OREF_INDEX_MASK;
            st.end = st.prim + ((ref >> OREF_COUNT_SHIFT) & OREF_COUNT_MASK) + 1u;
            st.slot = slot;
            if (wide) { // what is set aside: the root record with the mask of its other children, or the one other child itself
                uint32_t mask = 0;
                for (uint32_t k = 0; k < 4; ++k)
                    if (k != slot && (kids[k].second >> OREF_KIND_SHIFT) != OK_EMPTY) mask |= 1u << k;
                st.rest = mask;
                if (mask != 0u && (mask & (mask - 1u)) == 0u) {
                    const uint32_t other = kids[__builtin_ctz(mask)].second;
                    if ((other >> OREF_KIND_SHIFT) == OK_INNER) st.direct = other & OREF_INDEX_MASK;
                }
            } else {
                st.rest = kids[slot ^ 1u].second;
            }
            break;
        }
    }
    return st;
}

// Step 3, instance starts.  The same for a Translate / RotateY frame whose tree is a single leaf (a box's six faces in a flat leaf): a walk
// that enters the frame starts with the leaf's primitives; the visit of a root record with one child is skipped (Cornell: 2.6 of 9.2
// record visits per sample).  Returns the scene's instances with start_ref / start_box filled.
std::vector<Instance> instance_starts(const CompiledScene &cs, bool wide) {
    std::vector<Instance> instances = cs.instances;
    if (!cs.ordered) return instances;
    for (Instance &in : instances) {
        uint32_t only = 0, n = 0;
        const float *box = nullptr;
        auto look = [&](uint32_t ref, const float *b) { if ((ref >> OREF_KIND_SHIFT) != OK_EMPTY) { ++n; only = ref; box = b; } };
        if (wide) for (int k = 0; k < 4; ++k) look(cs.onodes4[in.root].c[k], cs.onodes4[in.root].b[k]);
        else { look(cs.onodes[in.root].c[0], cs.onodes[in.root].b0); look(cs.onodes[in.root].c[1], cs.onodes[in.root].b1); }
        const uint32_t kind = only >> OREF_KIND_SHIFT;
        in.start_ref = (n == 1 && (kind == OK_SPHERES || kind == OK_QUADS)) ? only : 0u;
        if (in.start_ref) memcpy(in.start_box, box, sizeof in.start_box);
    }
    return instances;
}

// Step 4, node tables (load_node / load_opair / load_oquad): threaded records as two 16-byte halves, the own trees' records as six plane
// tables and a reference table, with their global form beside them
NodeTables node_tables(const CompiledScene &cs) {
    if (cs.ordered && cs.wide) return pack_wide_records(cs.onodes4);
    const size_t n = cs.ordered ? cs.onodes.size() : cs.nodes32.size();
    const size_t off_b = n * 16; // bytes of one plane table (16 bytes per record)
    NodeTables nt;
    nt.table_bytes = off_b;
    nt.records = n;
    nt.tables.resize((cs.ordered ? align16(n * (6 * 16 + 8)) : n * 32) / 16);
    unsigned char *base = reinterpret_cast<unsigned char *>(nt.tables.data());
    if (!cs.ordered) {
        const unsigned char *src = reinterpret_cast<const unsigned char *>(cs.nodes32.data());
        for (size_t i = 0; i < n; ++i)
            for (size_t q = 0; q < 2; ++q) memcpy(base + q * off_b + i * 16, src + (i * 2 + q) * 16, 16);
        return nt;
    }
    for (size_t i = 0; i < n; ++i) {
        const ONode &nd = cs.onodes[i];
        for (int ax = 0; ax < 3; ++ax) {
            const float lo0 = nd.b0[2 * ax], hi0 = nd.b0[2 * ax + 1], lo1 = nd.b1[2 * ax], hi1 = nd.b1[2 * ax + 1];
            const float plus[4] = {lo0, lo1, hi0, hi1}, minus[4] = {hi0, hi1, lo0, lo1};
            memcpy(base + (size_t)(2 * ax) * off_b + i * 16, plus, 16);
            memcpy(base + (size_t)(2 * ax + 1) * off_b + i * 16, minus, 16);
        }
        memcpy(base + 6 * off_b + i * 8, nd.c, 8);
    }
    nt.lines.resize(n * 8); // the global copy: one 128-byte line per record (load_opair<0>)
    unsigned char *dst = reinterpret_cast<unsigned char *>(nt.lines.data());
    for (size_t i = 0; i < n; ++i) {
        for (size_t q = 0; q < 6; ++q) memcpy(dst + i * 128 + q * 16, base + q * off_b + i * 16, 16);
        memcpy(dst + i * 128 + 96, base + 6 * off_b + i * 8, 8);
    }
    return nt;
}

// Step 5, LDS image and level.  LDS image = node tables | spheres | quads | quad filter records; every LDS level copies a prefix.
// `walk`: the scene's walk_layout (what the stacks beside the image cost).
ScenePlan::Lds lds_image(const CompiledScene &cs, const NodeTables &nt, const Layout &walk, std::vector<uint4> &image) {
    ScenePlan::Lds lds;
    const size_t n = nt.records, off_sph = nt.tables.size() * 16;
    lds.off_node_b = (uint32_t)nt.table_bytes;
    const size_t off_quads = off_sph + cs.spheres.size() * sizeof(Sphere);
    // behind the quads: their f32 filter records (rt_qfilt.hpp) — if some leaf of the library's own trees holds more than one quad
    // (a single quad's exact test runs in its round anyway) and the LDS has room for them
    bool flat_quads = false;
    if (cs.ordered) {
        auto multi = [](uint32_t ref) { return (ref >> OREF_KIND_SHIFT) == OK_QUADS && ((ref >> OREF_COUNT_SHIFT) & OREF_COUNT_MASK) != 0u; };
        for (const ONode &nd : cs.onodes) flat_quads = flat_quads || multi(nd.c[0]) || multi(nd.c[1]);
        for (const ONode4 &nd : cs.onodes4) for (int k = 0; k < 4; ++k) flat_quads = flat_quads || multi(nd.c[k]);
    }
    const size_t off_qfilt = align16(off_quads + cs.quads.size() * sizeof(Quad));
    const size_t total_plain = off_qfilt, total_filt = off_qfilt + cs.quads.size() * sizeof(QFiltPair);
    const size_t stack3 = stack_bytes(walk, 3), stack1 = stack_bytes(walk, 1); // (the two levels' kernels differ in workgroup size)
    // level 2 (nodes + spheres) exists but is not selected: on final_scene it measured 10 % slower than level 1
    // (behind the stacks: the world's sequence, and the instrumented kernels' profile rows)
    const size_t budget = LDS_BUDGET_BYTES - 4096 - cs.oseq.size() * sizeof(OSeq);
    const bool with_filter = flat_quads && total_filt + stack3 <= budget;
    const size_t total = with_filter ? total_filt : total_plain;
    lds.level = total + stack3 <= budget ? 3 : (off_sph + stack1 <= budget ? 1 : 0);
    if (cs.ordered && n >= (cs.wide ? (size_t)WIDE_MAX_LDS_RECORDS : (size_t)0x3fffu)) lds.level = 0; // 2-byte stack entries: a record index in 14 bits + two skip bits (wide: 12 + 4 mask bits)
    if (!lds.level) return lds;
    const size_t used = lds.level == 3 ? total : (lds.level == 2 ? align16(off_quads) : off_sph);
    image.resize(used / 16);
    unsigned char *base = reinterpret_cast<unsigned char *>(image.data());
    memcpy(base, nt.tables.data(), off_sph);
    if (lds.level >= 2 && !cs.spheres.empty()) memcpy(base + off_sph, cs.spheres.data(), cs.spheres.size() * sizeof(Sphere));
    if (lds.level == 3 && !cs.quads.empty()) memcpy(base + off_quads, cs.quads.data(), cs.quads.size() * sizeof(Quad));
    if (lds.level == 3 && with_filter) {
        const std::vector<QFiltPair> qf = qfilt_table(cs.quads);
        memcpy(base + off_qfilt, qf.data(), qf.size() * sizeof(QFiltPair));
        lds.off_qfilt = (uint32_t)off_qfilt;
    }
    lds.off_spheres = (uint32_t)off_sph; lds.off_quads = (uint32_t)off_quads;
    lds.prefix_bytes[1] = (uint32_t)off_sph;
    lds.prefix_bytes[2] = (uint32_t)align16(off_quads);
    lds.prefix_bytes[3] = (uint32_t)total;
    for (int l = lds.level + 1; l < 4; ++l) lds.prefix_bytes[l] = 0;
    return lds;
}

// Step 6, materials (one entry more than the scene has materials: Color::ONE, what the path end multiplies by for a level a path does
// not have; two more where the one's index would be 0xffff, the mark of a parked colour)
std::vector<DMaterial> material_table(const CompiledScene &cs) {
    const size_t n_mats = cs.materials.size();
    std::vector<DMaterial> mats(n_mats + (n_mats == 0xffffu ? 2u : 1u));
    for (size_t i = n_mats; i < mats.size(); ++i) {
        mats[i].albedo[0] = mats[i].albedo[1] = mats[i].albedo[2] = 1.0;
        mats[i].solid = 1u;
    }
    for (size_t i = 0; i < n_mats; ++i) {
        const rt_material &m = cs.materials[i];
        DMaterial d{};
        d.kind = (uint32_t)m.kind;
        d.texture = m.texture >= 0 ? (uint32_t)m.texture : 0u;
        d.needs_uv = texture_needs_uv(cs.textures, m.texture) ? 1u : 0u;
        d.slow = (m.kind != RT_MATERIAL_METAL && m.kind != RT_MATERIAL_DIELECTRIC && texture_has_noise(cs.textures, m.texture)) ? 1u : 0u;
        d.albedo[0] = m.albedo.x; d.albedo[1] = m.albedo.y; d.albedo[2] = m.albedo.z;
        if (m.kind != RT_MATERIAL_METAL && m.kind != RT_MATERIAL_DIELECTRIC && m.texture >= 0 &&
            cs.textures[(size_t)m.texture].kind == RT_TEXTURE_SOLID) {
            const rt_vec3 &c = cs.textures[(size_t)m.texture].color;
            d.solid = 1u;
            d.albedo[0] = c.x; d.albedo[1] = c.y; d.albedo[2] = c.z;
        }
        d.fuzz = m.fuzz;
        d.ir = m.ir;
        if (m.kind == RT_MATERIAL_DIELECTRIC) {
            // a Dielectric attenuates by Color::ONE and reads no albedo: the three doubles carry what its scatter() divides out on every
            // hit (src/material.rs:86, :75-77) — the same IEEE operations, done once here: 1 / ir, and Schlick's r0 for either face
            const double inv_ir = 1.0 / m.ir;
            double r0_front = (1.0 - inv_ir) / (1.0 + inv_ir), r0_back = (1.0 - m.ir) / (1.0 + m.ir);
            r0_front = r0_front * r0_front; r0_back = r0_back * r0_back;
            d.albedo[0] = inv_ir; d.albedo[1] = r0_front; d.albedo[2] = r0_back;
        }
        mats[i] = d;
    }
    return mats;
}

// Step 7, AUX image (path_kernel's AUX): the small tables an ordered scene's kernel reads per hit — materials, frames, media, and
// (only when some texture is not a SolidColor: otherwise the colours sit in the material records) textures and Perlin
// tables; copied into the LDS wherever it fits (aux_in_lds)
ScenePlan::Aux aux_image(const CompiledScene &cs, const std::vector<DMaterial> &mats, const Layout &walk, std::vector<uint4> &image) {
    ScenePlan::Aux aux;
    const bool with_textures = (walk.features & F_TEXTURES) != 0;
    const size_t o_mats = 0, o_texs = align16(o_mats + mats.size() * sizeof(DMaterial)),
                 o_insts = align16(o_texs + (with_textures ? cs.textures.size() * sizeof(rt_texture) : 0u)),
                 o_media = align16(o_insts + cs.instances.size() * sizeof(Instance)),
                 o_perlins = align16(o_media + cs.media.size() * sizeof(Medium)),
                 total = align16(o_perlins + (with_textures ? cs.perlins.size() * sizeof(rt_perlin) : 0u));
    if (!(walk.ordered && total > 0 && total <= 48 * 1024)) return aux;
    image.resize(total / 16);
    unsigned char *base = reinterpret_cast<unsigned char *>(image.data());
    if (!mats.empty()) memcpy(base + o_mats, mats.data(), mats.size() * sizeof(DMaterial));
    if (with_textures && !cs.textures.empty()) memcpy(base + o_texs, cs.textures.data(), cs.textures.size() * sizeof(rt_texture));
    if (!cs.instances.empty()) memcpy(base + o_insts, cs.instances.data(), cs.instances.size() * sizeof(Instance));
    if (!cs.media.empty()) memcpy(base + o_media, cs.media.data(), cs.media.size() * sizeof(Medium));
    if (with_textures && !cs.perlins.empty()) memcpy(base + o_perlins, cs.perlins.data(), cs.perlins.size() * sizeof(rt_perlin));
    aux.bytes = (uint32_t)total;
    aux.off[0] = (uint32_t)o_mats; aux.off[1] = (uint32_t)o_texs; aux.off[2] = (uint32_t)o_insts;
    aux.off[3] = (uint32_t)o_media; aux.off[4] = (uint32_t)o_perlins;
    return aux;
}

template <class T> uint64_t bytes_of(const std::vector<T> &v) { return v.size() * sizeof(T); }

// rt_scene_get_stats, from the finished plan
rt_scene_stats scene_stats(const ScenePlan &p) {
    const CompiledScene &cs = p.cs;
    const Layout &l = p.layout;
    rt_scene_stats st{};
    st.node_bytes = cs.ordered ? bytes_of(p.oimage) : bytes_of(cs.nodes32); st.sphere_bytes = bytes_of(cs.spheres); st.quad_bytes = bytes_of(cs.quads);
    st.instance_bytes = bytes_of(cs.instances); st.medium_bytes = bytes_of(cs.media); st.material_bytes = bytes_of(p.mats);
    st.texture_bytes = bytes_of(cs.textures); st.perlin_bytes = bytes_of(cs.perlins); st.image_bytes = bytes_of(cs.texels);
    st.n_nodes = (uint32_t)(cs.ordered ? (cs.wide ? cs.onodes4.size() : cs.onodes.size()) : cs.nodes.size()); st.n_spheres = (uint32_t)cs.spheres.size(); st.n_quads = (uint32_t)cs.quads.size();
    st.n_instances = (uint32_t)cs.instances.size(); st.n_media = (uint32_t)cs.media.size();
    st.max_instance_depth = cs.max_instance_depth;
    st.lds_nodes = l.lds.level ? st.n_nodes : 0; st.lds_bytes = l.lds.level ? (uint32_t)dynamic_lds_bytes(l, l.lds.level, false) : 0;
    st.ordered = cs.ordered ? 1u : 0u; st.stack_entries = cs.ordered ? cs.ordered_stack : 0u;
    return st;
}

} // namespace

int plan_scene(const rt_scene_desc &desc, const rt_scene_options &resolved, const Tuning &tn, ScenePlan &out, const char *who) {
    ScenePlan p;
    if (int crc = compile_for_scene(desc, resolved, tn, p.cs, who)) return crc;
    try {
        Layout &l = p.layout;
        l = walk_layout(p.cs);
        l.start = start_shortcut(p.cs, l.wide, l.o_root);
        p.cs.instances = instance_starts(p.cs, l.wide);
        NodeTables nt = node_tables(p.cs);
        l.lds = lds_image(p.cs, nt, l, p.lds_image);
        p.oimage = std::move(nt.lines);
        p.mats = material_table(p.cs);
        l.aux = aux_image(p.cs, p.mats, l, p.aux_image);
        p.stats = scene_stats(p);
        out = std::move(p);
    } catch (const std::bad_alloc &) {
        return fail(RT_ERR_OUT_OF_MEMORY, std::string(who) + ": out of memory");
    } catch (const std::exception &e) {
        return fail(RT_ERR_INVALID_ARGUMENT, std::string(who) + ": " + e.what());
    }
    return RT_OK;
}

} // namespace rtapi
