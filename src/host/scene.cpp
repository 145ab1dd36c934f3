// src/host/scene.cpp -- Scene: flattens the caller's object graph into the arrays of include/pt_hip.h and owns the device scene.
#include <PathTrace/detail/world.h>
#include <PathTrace/gather.h>
#include <PathTrace/light_passes.h>
#include <PathTrace/light_probes.h>
#include <PathTrace/query.h>
#include <PathTrace/radiance.h>
#include <PathTrace/scene/mesh.h>

#include "../../include/pt_hip.h"
#include "job_params.h"

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdlib>
#include <map>
#include <mutex>
#include <random>
#include <stdexcept>
#include <string>
#include <thread>
#include <typeinfo>
#include <unordered_map>

namespace {

    void copy4(float *dst, const Color<float> &c) {
        for(int k = 0; k < 4; k++) {
            dst[k] = c[k];
        }
    }

    // the pt_material that describes `handler`
    pt_material describeMaterial(const MaterialHandler *handler) {
        const auto *constant = dynamic_cast<const ConstantMaterialHandler *>(handler);
        if(constant == nullptr) {
            throw std::invalid_argument("PathTrace: only ConstantMaterialHandler can be evaluated on the device");
        }
        const vec3<float> anywhere{0.0F, 0.0F, 0.0F};
        const Material *material = constant->getMaterial(anywhere);
        const BSDF *bsdf = constant->getBSDF(anywhere);
        if(dynamic_cast<const ConstantMaterial *>(material) == nullptr) {
            throw std::invalid_argument("PathTrace: only ConstantMaterial can be evaluated on the device");
        }
        pt_material m{};
        copy4(m.diffuse, material->getDiffuseColor(anywhere));
        copy4(m.specular, material->getSpecularColor(anywhere));
        copy4(m.emission, material->probeEmission().getColor());
        m.ior = material->getRefractiveIndex(anywhere);
        if(dynamic_cast<const LambertianBRDF *>(bsdf) != nullptr) {
            m.bsdf = PT_BSDF_LAMBERTIAN;
        }
        else if(dynamic_cast<const GlassBDF *>(bsdf) != nullptr) {
            m.bsdf = PT_BSDF_GLASS;
        }
        else if(const auto *mirror = dynamic_cast<const MirrorBRDF *>(bsdf)) {
            m.bsdf = PT_BSDF_MIRROR;
            m.one_way = mirror->isOneWay() ? 1 : 0;
        }
        else {
            throw std::invalid_argument("PathTrace: only LambertianBRDF, GlassBDF and MirrorBRDF can be evaluated on the device");
        }
        return m;
    }

    // index of the pt_material that describes `handler`, appending it on first use
    uint32_t materialIndex(const MaterialHandler *handler, std::map<const MaterialHandler *, uint32_t> &known, std::vector<pt_material> &materials) {
        auto found = known.find(handler);
        if(found != known.end()) {
            return found->second;
        }
        const pt_material m = describeMaterial(handler);
        const uint32_t index = static_cast<uint32_t>(materials.size());
        materials.push_back(m);
        known.emplace(handler, index);
        return index;
    }

    // position and spectrum of every light as the device takes them
    void describeLights(const std::vector<std::unique_ptr<LightSource>> &lights, std::vector<float> &light_pos, std::vector<float> &light_spectrum) {
        for(const auto &light : lights) {
            const auto *point = dynamic_cast<const PointLightSource *>(light.get());
            if(point == nullptr) {
                throw std::invalid_argument("PathTrace: only PointLightSource lights can be rendered on the device");
            }
            const vec3<float> anywhere{0.0F, 0.0F, 0.0F};
            const auto [target, density] = point->importanceSample(anywhere);
            (void)density;
            const auto colour = point->getSpectrum(Ray{anywhere, vec3<float>{0.0F, 0.0F, 1.0F}}).getColor();
            light_pos.insert(light_pos.end(), {target[0], target[1], target[2]});
            light_spectrum.insert(light_spectrum.end(), {colour[0], colour[1], colour[2], colour[3]});
        }
    }

    // What a Scene with mesh instances keeps beyond its data members (whose layout is fixed, detail/world.h): the instances, their object
    // ranges, and the Triangles handed out so far.
    struct MeshState {
        std::vector<MeshInstance> instances;
        std::vector<uint32_t> first, count; // object range of every instance
        std::vector<const MaterialHandler *> slots; // the handler behind every material index; one handler may hold several (Scene::relight)
        std::map<const io::MeshData *, uint32_t> skin_bones; // the bone count of the rig bound to a mesh (Scene::bindSkin)
        std::map<const io::MeshData *, uint32_t> morph_targets; // ... and the target count of its morph set (Scene::bindMorphs)
        std::mutex mutex;                   // guards `made`, `skin_bones` and `morph_targets`
        std::unordered_map<uint32_t, std::unique_ptr<Object>> made; // object index -> Triangle

        // The Triangle behind object `index`, made on first use from the arrays the device builder took
        const Object *object(pt_scene *device_scene, uint32_t index) {
            std::lock_guard<std::mutex> lock(mutex);
            auto found = made.find(index);
            if(found != made.end()) {
                return found->second.get();
            }
            float pos[9], nrm[9];
            uint8_t cull = 0;
            if(pt_scene_get_triangles(device_scene, index, 1, pos, nrm, &cull, nullptr) != PT_OK) {
                return nullptr;
            }
            auto triangle = std::make_unique<Triangle>(vec3<float>{pos[0], pos[1], pos[2]}, vec3<float>{pos[3], pos[4], pos[5]}, vec3<float>{pos[6], pos[7], pos[8]}, cull != 0);
            triangle->normal_a = vec3<float>{nrm[0], nrm[1], nrm[2]};
            triangle->normal_b = vec3<float>{nrm[3], nrm[4], nrm[5]};
            triangle->normal_c = vec3<float>{nrm[6], nrm[7], nrm[8]};
            const size_t instance = static_cast<size_t>(std::upper_bound(first.begin(), first.end(), index) - first.begin()) - 1;
            if(instances[instance].handler != nullptr) {
                triangle->setMaterialHandler(instances[instance].handler);
            }
            return made.emplace(index, std::move(triangle)).first->second.get();
        }
    };

    // The states of the Scenes that have one, by the Scene's address (a Scene is neither copied nor moved).  Never destroyed: a Scene
    // with static storage may outlive any static of this file.
    struct MeshStates {
        std::mutex mutex;
        std::unordered_map<const Scene *, std::unique_ptr<MeshState>> of;
    };
    MeshStates &meshStates() {
        static MeshStates *states = new MeshStates();
        return *states;
    }

} // namespace

Scene::Scene(std::vector<std::unique_ptr<Object>> &&objs, std::vector<std::unique_ptr<LightSource>> &&lights) :
  Scene(std::move(objs), std::move(lights), std::vector<MeshInstance>{}) {}

Scene::Scene(std::vector<std::unique_ptr<Object>> &&objs, std::vector<std::unique_ptr<LightSource>> &&lights, std::vector<MeshInstance> &&mesh_instances) :
  objects(std::move(objs)), light_sources(std::move(lights)) {
    // (registered under this Scene's address at the end, when nothing can throw any more)
    std::unique_ptr<MeshState> state;
    if(!mesh_instances.empty()) {
        state = std::make_unique<MeshState>();
        state->instances = std::move(mesh_instances);
    }
    const std::vector<MeshInstance> no_instances;
    const std::vector<MeshInstance> &instances = state != nullptr ? state->instances : no_instances;
    std::vector<uint8_t> kinds(objects.size());
    std::vector<float> tri_pos, tri_nrm, spheres, light_pos, light_spectrum;
    std::vector<uint8_t> tri_cull;
    std::vector<uint32_t> tri_material, sphere_material;
    std::vector<pt_material> materials;
    std::map<const MaterialHandler *, uint32_t> known;

    auto onAllCores = [](size_t count, auto body) { // body(first, last) over contiguous slices of [0, count)
        const size_t workers = count < 65536 ? 1 : std::min<size_t>(std::max(1U, std::thread::hardware_concurrency()), 64);
        if(workers == 1) {
            body(size_t{0}, count);
            return;
        }
        std::vector<std::thread> pool;
        for(size_t w = 0; w < workers; w++) {
            pool.emplace_back(body, count * w / workers, count * (w + 1) / workers);
        }
        for(auto &worker : pool) {
            worker.join();
        }
    };

    // pass 1, on all cores (the objects are scattered over the heap): dynamic type and material handler of every object
    std::vector<const MaterialHandler *> handler_of(objects.size());
    std::atomic<bool> unknown_kind{false};
    onAllCores(objects.size(), [&](size_t first, size_t last) {
        for(size_t i = first; i < last; i++) {
            const Object &object = *objects[i];
            handler_of[i] = object.getMaterialHandler();
            if(typeid(object) == typeid(Triangle)) { // both classes are final: the dynamic type is the class itself or something else
                kinds[i] = PT_OBJ_TRIANGLE;
            }
            else if(typeid(object) == typeid(Sphere)) {
                kinds[i] = PT_OBJ_SPHERE;
            }
            else {
                unknown_kind.store(true);
            }
        }
    });
    if(unknown_kind.load()) {
        throw std::invalid_argument("PathTrace: only Triangle and Sphere objects can be rendered on the device");
    }
    // ... then, in order, its position among the objects of its kind and its material index (meshes share one handler, so the
    // last one seen is remembered before the map is asked)
    std::vector<uint32_t> typed_index(objects.size()), material_of(objects.size());
    uint32_t n_triangles = 0, n_spheres = 0;
    {
        const MaterialHandler *last_handler = nullptr;
        uint32_t last_material = 0;
        bool have_last = false;
        for(size_t i = 0; i < objects.size(); i++) {
            if(!have_last || handler_of[i] != last_handler) {
                last_material = materialIndex(handler_of[i], known, materials);
                last_handler = handler_of[i];
                have_last = true;
            }
            material_of[i] = last_material;
            typed_index[i] = kinds[i] == PT_OBJ_TRIANGLE ? n_triangles++ : n_spheres++;
        }
    }
    // pass 2, on all cores: the coordinate arrays
    tri_pos.resize(9 * static_cast<size_t>(n_triangles));
    tri_nrm.resize(9 * static_cast<size_t>(n_triangles));
    tri_cull.resize(n_triangles);
    tri_material.resize(n_triangles);
    spheres.resize(4 * static_cast<size_t>(n_spheres));
    sphere_material.resize(n_spheres);
    {
        auto fill = [&](size_t first, size_t last) {
            for(size_t i = first; i < last; i++) {
                const size_t k = typed_index[i];
                if(kinds[i] == PT_OBJ_TRIANGLE) {
                    const auto *t = static_cast<const Triangle *>(objects[i].get());
                    const vec3<float> *points[3] = {&t->a, &t->b, &t->c};
                    const vec3<float> *normals[3] = {&t->normal_a, &t->normal_b, &t->normal_c};
                    for(int v = 0; v < 3; v++) {
                        for(int c = 0; c < 3; c++) {
                            tri_pos[9 * k + 3 * static_cast<size_t>(v) + static_cast<size_t>(c)] = (*points[v])[static_cast<size_t>(c)];
                            tri_nrm[9 * k + 3 * static_cast<size_t>(v) + static_cast<size_t>(c)] = (*normals[v])[static_cast<size_t>(c)];
                        }
                    }
                    tri_cull[k] = t->cullsBackface() ? 1 : 0;
                    tri_material[k] = material_of[i];
                }
                else {
                    const auto *sphere = static_cast<const Sphere *>(objects[i].get());
                    const auto o = sphere->getOrigin();
                    spheres[4 * k + 0] = o[0];
                    spheres[4 * k + 1] = o[1];
                    spheres[4 * k + 2] = o[2];
                    spheres[4 * k + 3] = sphere->getRadius();
                    sphere_material[k] = material_of[i];
                }
            }
        };
        onAllCores(objects.size(), fill);
    }
    describeLights(light_sources, light_pos, light_spectrum);

    pt_scene_desc desc{};
    desc.n_objects = static_cast<uint32_t>(kinds.size());
    desc.obj_kind = kinds.data();
    desc.n_triangles = static_cast<uint32_t>(tri_cull.size());
    desc.tri_pos = tri_pos.data();
    desc.tri_nrm = tri_nrm.data();
    desc.tri_cull = tri_cull.data();
    desc.tri_material = tri_material.data();
    desc.n_spheres = static_cast<uint32_t>(sphere_material.size());
    desc.sph = spheres.data();
    desc.sph_material = sphere_material.data();
    desc.n_materials = static_cast<uint32_t>(materials.size());
    desc.materials = materials.data();
    desc.n_point_lights = static_cast<uint32_t>(light_sources.size());
    desc.light_pos = light_pos.data();
    desc.light_spectrum = light_spectrum.data();

    // the mesh instances: every MeshData once, and per instance its matrix, flags and material
    static_assert(sizeof(vec3<float>) == 3 * sizeof(float) && sizeof(std::array<int32_t, 3>) == 3 * sizeof(int32_t), "MeshData is handed over as flat arrays");
    std::vector<pt_mesh_data> mesh_data;
    std::vector<pt_mesh_instance> mesh_instances_flat(instances.size());
    {
        std::map<const io::MeshData *, uint32_t> mesh_of;
        for(size_t i = 0; i < instances.size(); i++) {
            const MeshInstance &instance = instances[i];
            if(instance.mesh == nullptr) {
                throw std::invalid_argument("PathTrace: a MeshInstance without a mesh");
            }
            auto found = mesh_of.find(instance.mesh.get());
            if(found == mesh_of.end()) {
                pt_mesh_data data{};
                data.n_vertices = static_cast<uint32_t>(instance.mesh->vertices.size());
                data.vertices = reinterpret_cast<const float *>(instance.mesh->vertices.data());
                data.n_faces = static_cast<uint32_t>(instance.mesh->faces.size());
                data.faces = reinterpret_cast<const int32_t *>(instance.mesh->faces.data());
                found = mesh_of.emplace(instance.mesh.get(), static_cast<uint32_t>(mesh_data.size())).first;
                mesh_data.push_back(data);
            }
            pt_mesh_instance &flat = mesh_instances_flat[i];
            flat.mesh = found->second;
            for(int r = 0; r < 4; r++) {
                for(int c = 0; c < 4; c++) {
                    flat.transform[4 * r + c] = instance.transformation.rows[r][c];
                }
            }
            flat.smooth = instance.smooth ? 1 : 0;
            flat.cull_backface = instance.cull_backface ? 1 : 0;
            flat.material = instance.handler != nullptr ? materialIndex(instance.handler.get(), known, materials) : PT_NO_MATERIAL;
        }
        desc.n_materials = static_cast<uint32_t>(materials.size());
        desc.materials = materials.data();
    }

    const char *device_env = std::getenv("PATHTRACE_DEVICE");
    const int device = device_env != nullptr ? std::atoi(device_env) : 0;
    int n_replicas = 1;
    if(const char *devices_env = std::getenv("PATHTRACE_DEVICES")) {
        n_replicas = std::string(devices_env) == "all" ? pt_device_count() - device : std::atoi(devices_env);
        n_replicas = std::max(n_replicas, 1);
    }
    // (tests on a one-GPU box: $PATHTRACE_REPLICAS_SHARE_DEVICE = k makes k replicas on the first device)
    int share = 0;
    if(const char *share_env = std::getenv("PATHTRACE_REPLICAS_SHARE_DEVICE")) {
        share = std::atoi(share_env);
        n_replicas = std::max(n_replicas, share);
    }
    for(int r = 0; r < n_replicas; r++) {
        pt_scene *replica = nullptr;
        if(pt_scene_create_meshes(share > 0 ? device : device + r, &desc, mesh_data.data(), static_cast<uint32_t>(mesh_data.size()), mesh_instances_flat.data(),
                                  static_cast<uint32_t>(mesh_instances_flat.size()), &replica) != PT_OK) {
            const std::string message = pt_last_error();
            for(pt_scene *made : replicas) {
                pt_scene_destroy(made);
            }
            replicas.clear();
            throw std::runtime_error("PathTrace: cannot create the device scene on device " + std::to_string(device + r) + ": " + message);
        }
        replicas.push_back(replica);
    }
    device_scene = replicas[0];
    if(state != nullptr) {
        state->first.resize(instances.size());
        state->count.resize(instances.size());
        pt_scene_instance_ranges(device_scene, state->first.data(), state->count.data());
        state->slots.assign(materials.size(), nullptr);
        for(const auto &[handler, index] : known) {
            state->slots[index] = handler;
        }
    }

    // (the emitters among the mesh triangles are materialised through the state, which is registered first; nothing below throws)
    if(state != nullptr) {
        MeshStates &states = meshStates();
        std::lock_guard<std::mutex> lock(states.mutex);
        states.of[this] = std::move(state);
    }
    registerEmitters();
}

// emissive objects and their cumulative selection probabilities, in the order the hierarchy registers them
void Scene::registerEmitters() {
    uint64_t n_emissive = 0;
    pt_scene_emissive(device_scene, nullptr, nullptr, 0, &n_emissive);
    std::vector<int32_t> indices(n_emissive);
    emissive.clear();
    emissive_cdf.assign(n_emissive, 0.0F);
    pt_scene_emissive(device_scene, indices.data(), emissive_cdf.data(), n_emissive, nullptr);
    for(int32_t i : indices) {
        emissive.push_back(static_cast<size_t>(i) < objects.size() ? objects[static_cast<size_t>(i)].get() : meshObject(static_cast<uint32_t>(i)));
    }
}

void Scene::pose(const std::vector<mat4<float>> &transformations) {
    std::vector<uint32_t> all(transformations.size());
    for(size_t i = 0; i < all.size(); i++) {
        all[i] = static_cast<uint32_t>(i);
    }
    MeshState *state = nullptr;
    {
        MeshStates &states = meshStates();
        std::lock_guard<std::mutex> lock(states.mutex);
        auto found = states.of.find(this);
        state = found != states.of.end() ? found->second.get() : nullptr;
    }
    if(state != nullptr && transformations.size() != state->instances.size()) {
        throw std::invalid_argument("PathTrace: Scene::pose needs one transformation per mesh instance");
    }
    pose(all, transformations);
}

void Scene::pose(const std::vector<uint32_t> &instances, const std::vector<mat4<float>> &transformations) {
    MeshState *state = nullptr;
    {
        MeshStates &states = meshStates();
        std::lock_guard<std::mutex> lock(states.mutex);
        auto found = states.of.find(this);
        state = found != states.of.end() ? found->second.get() : nullptr;
    }
    if(state == nullptr) {
        throw std::invalid_argument("PathTrace: Scene::pose on a Scene without mesh instances");
    }
    if(instances.size() != transformations.size()) {
        throw std::invalid_argument("PathTrace: Scene::pose needs one transformation per named instance");
    }
    for(uint32_t i : instances) {
        if(i >= state->instances.size()) {
            throw std::invalid_argument("PathTrace: Scene::pose names an instance that is not there");
        }
    }
    if(instances.empty()) {
        return;
    }
    std::vector<float> flat(16 * transformations.size());
    for(size_t k = 0; k < transformations.size(); k++) {
        for(int r = 0; r < 4; r++) {
            for(int c = 0; c < 4; c++) {
                flat[16 * k + 4 * static_cast<size_t>(r) + static_cast<size_t>(c)] = transformations[k].rows[r][c];
            }
        }
    }
    for(size_t r = 0; r < replicas.size(); r++) {
        if(pt_scene_pose(replicas[r], instances.data(), static_cast<uint32_t>(instances.size()), flat.data(), nullptr) != PT_OK) {
            throw std::runtime_error("PathTrace: cannot pose the device scene (replica " + std::to_string(r) + "): " + pt_last_error());
        }
    }
    {
        std::lock_guard<std::mutex> lock(state->mutex);
        for(size_t k = 0; k < instances.size(); k++) {
            state->instances[instances[k]].transformation = transformations[k];
        }
        pt_scene_instance_ranges(device_scene, state->first.data(), state->count.data());
        state->made.clear(); // (the Triangles handed out so far: their objects are other triangles now, or none)
    }
    registerEmitters();
}

void Scene::relight(const std::vector<std::pair<std::shared_ptr<MaterialHandler>, std::shared_ptr<MaterialHandler>>> &replace) {
    MeshState *state = nullptr;
    {
        MeshStates &states = meshStates();
        std::lock_guard<std::mutex> lock(states.mutex);
        auto found = states.of.find(this);
        state = found != states.of.end() ? found->second.get() : nullptr;
    }
    if(state == nullptr) {
        throw std::invalid_argument("PathTrace: Scene::relight on a Scene without mesh instances");
    }
    if(replace.empty()) {
        return;
    }
    uint32_t n_materials = 0;
    if(pt_scene_get_materials(device_scene, nullptr, 0, &n_materials) != PT_OK) {
        throw std::runtime_error(std::string("PathTrace: cannot read the device scene's materials: ") + pt_last_error());
    }
    std::vector<pt_material> materials(n_materials);
    pt_scene_get_materials(device_scene, materials.data(), n_materials, nullptr);
    // every replacement takes the slot of the handler it replaces (checked and described before anything changes)
    std::vector<const MaterialHandler *> slots = state->slots;
    for(const auto &[from, to] : replace) {
        if(from == nullptr || to == nullptr || std::find(slots.begin(), slots.end(), from.get()) == slots.end()) {
            throw std::invalid_argument("PathTrace: Scene::relight replaces a handler the Scene does not use");
        }
        const pt_material described = describeMaterial(to.get());
        // (a handler may hold several slots: it took over those of the handlers it replaced earlier; all of them follow it)
        for(size_t slot = 0; slot < slots.size() && slot < materials.size(); slot++) {
            if(slots[slot] == from.get()) {
                materials[slot] = described;
                slots[slot] = to.get();
            }
        }
    }
    pt_relight look{};
    look.materials = materials.data();
    look.n_materials = n_materials;
    for(size_t r = 0; r < replicas.size(); r++) {
        if(pt_scene_relight(replicas[r], &look, nullptr) != PT_OK) {
            throw std::runtime_error("PathTrace: cannot relight the device scene (replica " + std::to_string(r) + "): " + pt_last_error());
        }
    }
    {
        std::lock_guard<std::mutex> lock(state->mutex);
        for(const auto &[from, to] : replace) {
            for(auto &object : objects) {
                if(object->getMaterialHandler() == from.get()) {
                    object->setMaterialHandler(to);
                }
            }
            for(MeshInstance &instance : state->instances) {
                if(instance.handler == from) {
                    instance.handler = to;
                }
            }
        }
        state->slots = std::move(slots);
        state->made.clear(); // (the Triangles handed out so far carry the handlers from before)
    }
    registerEmitters();
}

void Scene::relight(std::vector<std::unique_ptr<LightSource>> &&new_light_sources) {
    {
        MeshStates &states = meshStates();
        std::lock_guard<std::mutex> lock(states.mutex);
        if(states.of.find(this) == states.of.end()) {
            throw std::invalid_argument("PathTrace: Scene::relight on a Scene without mesh instances");
        }
    }
    std::vector<float> light_pos, light_spectrum;
    describeLights(new_light_sources, light_pos, light_spectrum);
    pt_relight look{};
    look.set_point_lights = 1;
    look.light_pos = light_pos.data();
    look.light_spectrum = light_spectrum.data();
    look.n_point_lights = static_cast<uint32_t>(new_light_sources.size());
    for(size_t r = 0; r < replicas.size(); r++) {
        if(pt_scene_relight(replicas[r], &look, nullptr) != PT_OK) {
            throw std::runtime_error("PathTrace: cannot relight the device scene (replica " + std::to_string(r) + "): " + pt_last_error());
        }
    }
    light_sources = std::move(new_light_sources);
    registerEmitters();
}

namespace {

    MeshState *meshStateOf(const Scene *scene, const char *who) {
        MeshStates &states = meshStates();
        std::lock_guard<std::mutex> lock(states.mutex);
        auto found = states.of.find(scene);
        if(found == states.of.end()) {
            throw std::invalid_argument(std::string("PathTrace: Scene::") + who + " on a Scene without mesh instances");
        }
        return found->second.get();
    }

    // The index the constructor gave `mesh` in the device scene's mesh list: MeshData are numbered in the order the instances first use them
    uint32_t meshIndexOf(const MeshState &state, const io::MeshData *mesh, const char *who) {
        std::map<const io::MeshData *, uint32_t> mesh_of;
        for(const MeshInstance &instance : state.instances) {
            mesh_of.emplace(instance.mesh.get(), static_cast<uint32_t>(mesh_of.size()));
        }
        auto found = mesh_of.find(mesh);
        if(mesh == nullptr || found == mesh_of.end()) {
            throw std::invalid_argument(std::string("PathTrace: Scene::") + who + " names a mesh no instance of the Scene uses");
        }
        return found->second;
    }

    // One pt_mesh_deform on every replica, then what a pose leaves to do on the host side: the ranges, and the Triangles handed out so far
    void deformReplicas(const std::vector<pt_scene *> &replicas, MeshState &state, const pt_mesh_deform &deform, const char *who) {
        for(size_t r = 0; r < replicas.size(); r++) {
            const int rc = pt_scene_deform(replicas[r], &deform, 1, nullptr, 0, nullptr, nullptr);
            if(rc != PT_OK) {
                throw std::runtime_error(std::string("PathTrace: Scene::") + who + " cannot deform the device scene (replica " + std::to_string(r) + "): " + pt_last_error());
            }
        }
        std::lock_guard<std::mutex> lock(state.mutex);
        pt_scene_instance_ranges(replicas[0], state.first.data(), state.count.data());
        state.made.clear(); // (the Triangles handed out so far: their objects are other triangles now, or none)
    }

} // namespace

void Scene::bindSkin(const std::shared_ptr<const io::MeshData> &mesh, const std::vector<uint32_t> &bone_indices, const std::vector<float> &weights, uint32_t influences) {
    MeshState *state = meshStateOf(this, "bindSkin");
    pt_skin skin{};
    skin.mesh = meshIndexOf(*state, mesh.get(), "bindSkin");
    if(influences < 1 || influences > PT_SKIN_MAX_INFLUENCES) {
        throw std::invalid_argument("PathTrace: Scene::bindSkin takes 1 .. 8 influences per vertex");
    }
    if(bone_indices.size() != mesh->vertices.size() * influences || weights.size() != bone_indices.size()) {
        throw std::invalid_argument("PathTrace: Scene::bindSkin needs `influences` bone indices and weights per vertex of the mesh");
    }
    skin.n_bones = bone_indices.empty() ? 1 : *std::max_element(bone_indices.begin(), bone_indices.end()) + 1;
    skin.influences = influences;
    const uint32_t no_index = 0;
    const float no_weight = 0.0F;
    skin.bone = bone_indices.empty() ? &no_index : bone_indices.data(); // (a mesh without vertices: a null array would unbind)
    skin.weight = weights.empty() ? &no_weight : weights.data();
    for(size_t r = 0; r < replicas.size(); r++) {
        const int rc = pt_scene_bind_skin(replicas[r], &skin);
        if(rc != PT_OK) {
            throw std::runtime_error("PathTrace: Scene::bindSkin cannot bind the skin (replica " + std::to_string(r) + "): " + pt_last_error());
        }
    }
    std::lock_guard<std::mutex> lock(state->mutex);
    state->skin_bones[mesh.get()] = skin.n_bones;
}

void Scene::deform(const std::shared_ptr<const io::MeshData> &mesh, const std::vector<vec3<float>> &vertices) {
    static_assert(sizeof(vec3<float>) == 3 * sizeof(float), "vertices are handed over as a flat array");
    MeshState *state = meshStateOf(this, "deform");
    pt_mesh_deform deform{};
    deform.mesh = meshIndexOf(*state, mesh.get(), "deform");
    deform.kind = PT_DEFORM_VERTICES;
    if(vertices.size() != mesh->vertices.size()) {
        throw std::invalid_argument("PathTrace: Scene::deform needs one vertex per vertex of the mesh");
    }
    const float none[3] = {0.0F, 0.0F, 0.0F};
    deform.data = vertices.empty() ? none : reinterpret_cast<const float *>(vertices.data());
    deform.count = static_cast<uint32_t>(vertices.size());
    deformReplicas(replicas, *state, deform, "deform");
    registerEmitters();
}

void Scene::deform(const std::shared_ptr<const io::MeshData> &mesh, const std::vector<mat4<float>> &bones) {
    MeshState *state = meshStateOf(this, "deform");
    pt_mesh_deform deform{};
    deform.mesh = meshIndexOf(*state, mesh.get(), "deform");
    deform.kind = PT_DEFORM_BONES;
    {
        std::lock_guard<std::mutex> lock(state->mutex);
        auto bound = state->skin_bones.find(mesh.get());
        if(bound == state->skin_bones.end()) {
            throw std::invalid_argument("PathTrace: Scene::deform with bones needs a rig (Scene::bindSkin first)");
        }
        if(bones.size() != bound->second) {
            throw std::invalid_argument("PathTrace: Scene::deform needs one matrix per bone of the rig");
        }
    }
    std::vector<float> rows(12 * std::max<size_t>(bones.size(), 1));
    for(size_t b = 0; b < bones.size(); b++) {
        for(int r = 0; r < 3; r++) {
            for(int c = 0; c < 4; c++) {
                rows[12 * b + 4 * static_cast<size_t>(r) + static_cast<size_t>(c)] = bones[b].rows[r][c];
            }
        }
    }
    deform.data = rows.data();
    deform.count = static_cast<uint32_t>(bones.size());
    deformReplicas(replicas, *state, deform, "deform");
    registerEmitters();
}

void Scene::restShape(const std::shared_ptr<const io::MeshData> &mesh) {
    MeshState *state = meshStateOf(this, "restShape");
    pt_mesh_deform deform{};
    deform.mesh = meshIndexOf(*state, mesh.get(), "restShape");
    deform.kind = PT_DEFORM_REST;
    deformReplicas(replicas, *state, deform, "restShape");
    registerEmitters();
}

void Scene::markMotion() {
    meshStateOf(this, "markMotion");
    for(size_t r = 0; r < replicas.size(); r++) {
        if(pt_scene_motion_mark(replicas[r], nullptr) != PT_OK) {
            throw std::runtime_error("PathTrace: Scene::markMotion cannot mark the device scene (replica " + std::to_string(r) + "): " + pt_last_error());
        }
    }
}

void Scene::unmarkMotion() {
    meshStateOf(this, "unmarkMotion");
    for(size_t r = 0; r < replicas.size(); r++) {
        if(pt_scene_motion_unmark(replicas[r]) != PT_OK) {
            throw std::runtime_error("PathTrace: Scene::unmarkMotion cannot unmark the device scene (replica " + std::to_string(r) + "): " + pt_last_error());
        }
    }
}

void Scene::bindMorphs(const std::shared_ptr<const io::MeshData> &mesh, const std::vector<MorphTarget> &targets) {
    static_assert(sizeof(vec3<float>) == 3 * sizeof(float), "deltas are handed over as a flat array");
    MeshState *state = meshStateOf(this, "bindMorphs");
    pt_morph_set set{};
    set.mesh = meshIndexOf(*state, mesh.get(), "bindMorphs");
    const size_t n_vertices = mesh->vertices.size();
    std::vector<pt_morph_target> table(targets.size());
    const uint32_t no_index = 0;
    const float no_delta[3] = {0.0F, 0.0F, 0.0F};
    for(size_t t = 0; t < targets.size(); t++) {
        const MorphTarget &target = targets[t];
        const bool dense = target.vertices.empty();
        if(dense ? (!target.deltas.empty() && target.deltas.size() != n_vertices) : target.deltas.size() != target.vertices.size()) {
            throw std::invalid_argument("PathTrace: Scene::bindMorphs needs one delta per listed vertex, or, without indices, per vertex of the mesh");
        }
        for(size_t j = 0; j < target.vertices.size(); j++) {
            if(target.vertices[j] >= n_vertices || (j > 0 && target.vertices[j] <= target.vertices[j - 1])) {
                throw std::invalid_argument("PathTrace: Scene::bindMorphs needs strictly ascending vertex indices below the mesh's vertex count");
            }
        }
        table[t].n_deltas = static_cast<uint32_t>(target.deltas.size());
        // (an empty target keeps a non-null index array: without indices it would be a dense one)
        table[t].vertex = dense ? (target.deltas.empty() ? &no_index : nullptr) : target.vertices.data();
        table[t].delta = target.deltas.empty() ? no_delta : reinterpret_cast<const float *>(target.deltas.data());
    }
    set.n_targets = static_cast<uint32_t>(table.size());
    set.targets = table.empty() ? nullptr : table.data();
    for(size_t r = 0; r < replicas.size(); r++) {
        const int rc = pt_scene_bind_morphs(replicas[r], &set);
        if(rc != PT_OK) {
            throw std::runtime_error("PathTrace: Scene::bindMorphs cannot bind the targets (replica " + std::to_string(r) + "): " + pt_last_error());
        }
    }
    std::lock_guard<std::mutex> lock(state->mutex);
    state->morph_targets[mesh.get()] = set.n_targets;
}

namespace {

    // One pt_mesh_morph on every replica, then what a deform leaves to do on the host side
    void morphReplicas(const std::vector<pt_scene *> &replicas, MeshState &state, const io::MeshData *mesh, pt_mesh_morph &morph, const std::vector<float> &weights) {
        {
            std::lock_guard<std::mutex> lock(state.mutex);
            auto bound = state.morph_targets.find(mesh);
            if(bound == state.morph_targets.end() || bound->second == 0) {
                throw std::invalid_argument("PathTrace: Scene::morph needs bound targets (Scene::bindMorphs first)");
            }
            if(weights.size() != bound->second) {
                throw std::invalid_argument("PathTrace: Scene::morph needs one weight per bound target");
            }
        }
        morph.weights = weights.data();
        morph.n_weights = static_cast<uint32_t>(weights.size());
        for(size_t r = 0; r < replicas.size(); r++) {
            const int rc = pt_scene_morph(replicas[r], &morph, 1, nullptr, 0, nullptr, nullptr);
            if(rc != PT_OK) {
                throw std::runtime_error("PathTrace: Scene::morph cannot morph the device scene (replica " + std::to_string(r) + "): " + pt_last_error());
            }
        }
        std::lock_guard<std::mutex> lock(state.mutex);
        pt_scene_instance_ranges(replicas[0], state.first.data(), state.count.data());
        state.made.clear(); // (the Triangles handed out so far: their objects are other triangles now, or none)
    }

} // namespace

void Scene::morph(const std::shared_ptr<const io::MeshData> &mesh, const std::vector<float> &weights) {
    MeshState *state = meshStateOf(this, "morph");
    pt_mesh_morph morph{};
    morph.mesh = meshIndexOf(*state, mesh.get(), "morph");
    morphReplicas(replicas, *state, mesh.get(), morph, weights);
    registerEmitters();
}

void Scene::morph(const std::shared_ptr<const io::MeshData> &mesh, const std::vector<float> &weights, const std::vector<mat4<float>> &bones) {
    MeshState *state = meshStateOf(this, "morph");
    pt_mesh_morph morph{};
    morph.mesh = meshIndexOf(*state, mesh.get(), "morph");
    {
        std::lock_guard<std::mutex> lock(state->mutex);
        auto bound = state->skin_bones.find(mesh.get());
        if(bound == state->skin_bones.end()) {
            throw std::invalid_argument("PathTrace: Scene::morph with bones needs a rig (Scene::bindSkin first)");
        }
        if(bones.size() != bound->second) {
            throw std::invalid_argument("PathTrace: Scene::morph needs one matrix per bone of the rig");
        }
    }
    std::vector<float> rows(12 * std::max<size_t>(bones.size(), 1));
    for(size_t b = 0; b < bones.size(); b++) {
        for(int r = 0; r < 3; r++) {
            for(int c = 0; c < 4; c++) {
                rows[12 * b + 4 * static_cast<size_t>(r) + static_cast<size_t>(c)] = bones[b].rows[r][c];
            }
        }
    }
    morph.bones = rows.data();
    morph.n_bones = static_cast<uint32_t>(bones.size());
    morphReplicas(replicas, *state, mesh.get(), morph, weights);
    registerEmitters();
}

// The Triangle behind object `index` of a mesh instance (MeshState::object)
size_t pathtrace_host::sceneInstanceCount(const Scene &scene) {
    MeshStates &states = meshStates();
    std::lock_guard<std::mutex> lock(states.mutex);
    auto found = states.of.find(&scene);
    return found != states.of.end() ? found->second->instances.size() : 0;
}

const Object *Scene::meshObject(uint32_t index) const {
    MeshState *state = nullptr;
    {
        MeshStates &states = meshStates();
        std::lock_guard<std::mutex> lock(states.mutex);
        auto found = states.of.find(this);
        if(found != states.of.end()) {
            state = found->second.get();
        }
    }
    return state != nullptr ? state->object(device_scene, index) : nullptr;
}

Scene::~Scene() {
    {
        MeshStates &states = meshStates();
        std::lock_guard<std::mutex> lock(states.mutex);
        states.of.erase(this);
    }
    for(pt_scene *replica : replicas) {
        pt_scene_destroy(replica);
    }
}

std::tuple<float, const Object *> Scene::getIntersection(const Ray &ray) const noexcept {
    const float packed[6] = {ray.origin[0], ray.origin[1], ray.origin[2], ray.dir[0], ray.dir[1], ray.dir[2]};
    float t = -1.0F;
    int32_t index = -1;
    if(pt_intersect_batch(device_scene, packed, 1, &t, &index) != PT_OK || index < 0) {
        return {t < 0.0F ? t : -1.0F, nullptr};
    }
    if(static_cast<size_t>(index) >= objects.size()) {
        const Object *object = meshObject(static_cast<uint32_t>(index));
        return {object != nullptr ? t : -1.0F, object};
    }
    return {t, objects[static_cast<size_t>(index)].get()};
}

PickResult Scene::pick(const Camera &camera, const RenderOptions &options, int x, int y) const {
    if(x < 0 || y < 0 || x >= options.image_width || y >= options.image_height) {
        throw std::invalid_argument("PathTrace: Scene::pick: the pixel lies outside the frame");
    }
    const pt_camera_params cam = pathtrace_host::cameraParams(camera);
    const pt_options opt = pathtrace_host::renderOptions(options);
    const int32_t xy[2] = {x, y};
    pt_hit h{};
    pathtrace_host::check(pt_query_pixels(device_scene, &cam, &opt, xy, 1, &h), "Scene::pick");
    PickResult out;
    if(h.object < 0) {
        return out;
    }
    out.object = static_cast<size_t>(h.object) >= objects.size() ? meshObject(static_cast<uint32_t>(h.object)) : objects[static_cast<size_t>(h.object)].get();
    if(out.object == nullptr) {
        return out;
    }
    out.hit = true;
    out.t = h.t;
    out.object_index = h.object;
    out.instance = h.instance;
    out.face = h.face;
    out.position = vec3<float>{h.position[0], h.position[1], h.position[2]};
    out.normal = vec3<float>{h.normal[0], h.normal[1], h.normal[2]};
    out.geometric_normal = vec3<float>{h.geometric_normal[0], h.geometric_normal[1], h.geometric_normal[2]};
    out.b1 = h.b1;
    out.b2 = h.b2;
    return out;
}

bool Scene::occluded(const Ray &ray, float t_max) const {
    const float segment[7] = {ray.origin[0], ray.origin[1], ray.origin[2], ray.dir[0], ray.dir[1], ray.dir[2], t_max};
    uint8_t blocked = 0;
    pathtrace_host::check(pt_occluded_rays(device_scene, segment, 1, &blocked), "Scene::occluded");
    return blocked != 0;
}

namespace {

    // The parameters of the C ABI; what it would refuse is refused here, as an argument error
    pt_gather_params gatherParams(const GatherOptions &o, const char *what) {
        if(o.samples < 1 || !(o.epsilon >= 0.0F) || (o.kind == GatherKind::occlusion && !(o.distance > 0.0F)) ||
           (o.kind != GatherKind::occlusion && o.kind != GatherKind::direct && o.kind != GatherKind::paths)) {
            throw std::invalid_argument(std::string("PathTrace: ") + what + ": samples must be at least 1, epsilon not negative, an occlusion distance positive and the kind known");
        }
        pt_gather_params p{};
        p.kind = static_cast<int32_t>(o.kind);
        p.samples = o.samples;
        p.epsilon = o.epsilon;
        p.distance = o.distance;
        p.base_seed = o.base_seed;
        return p;
    }

    GatherResult gatherResult(const pt_gather_result &r) {
        GatherResult out;
        out.value = Color<float>{r.value[0], r.value[1], r.value[2], r.value[3]};
        out.samples = r.samples;
        out.occluded = r.occluded;
        return out;
    }

} // namespace

std::vector<GatherResult> Scene::gather(const std::vector<GatherPoint> &points, const GatherOptions &gather_options) const {
    const pt_gather_params params = gatherParams(gather_options, "Scene::gather");
    std::vector<float> packed(6 * points.size());
    for(size_t i = 0; i < points.size(); i++) {
        for(size_t k = 0; k < 3; k++) {
            packed[6 * i + k] = points[i].position[k];
            packed[6 * i + 3 + k] = points[i].normal[k];
        }
    }
    std::vector<pt_gather_result> raw(points.size());
    pathtrace_host::check(pt_gather_points(device_scene, packed.data(), points.size(), &params, raw.data()), "Scene::gather");
    std::vector<GatherResult> out(points.size());
    std::transform(raw.begin(), raw.end(), out.begin(), gatherResult);
    return out;
}

std::vector<GatherResult> Scene::gatherFrame(const Camera &camera, const RenderOptions &options, const GatherOptions &gather_options) const {
    const pt_gather_params params = gatherParams(gather_options, "Scene::gatherFrame");
    if(options.image_width <= 0 || options.image_height <= 0) {
        throw std::invalid_argument("PathTrace: Scene::gatherFrame: the image size must be positive");
    }
    const pt_camera_params cam = pathtrace_host::cameraParams(camera);
    const pt_options opt = pathtrace_host::renderOptions(options);
    std::vector<pt_gather_result> raw(static_cast<size_t>(options.image_width) * static_cast<size_t>(options.image_height));
    pathtrace_host::check(pt_gather_frame(device_scene, &cam, &opt, &params, raw.data()), "Scene::gatherFrame");
    std::vector<GatherResult> out(raw.size());
    std::transform(raw.begin(), raw.end(), out.begin(), gatherResult);
    return out;
}

std::vector<std::array<GatherResult, 3>> Scene::bakeInstance(size_t instance, const GatherOptions &gather_options) const {
    const pt_gather_params params = gatherParams(gather_options, "Scene::bakeInstance");
    const size_t n_instances = pathtrace_host::sceneInstanceCount(*this);
    if(instance >= n_instances) {
        throw std::invalid_argument("PathTrace: Scene::bakeInstance: instance out of range");
    }
    std::vector<uint32_t> first(n_instances), count(n_instances);
    pathtrace_host::check(pt_scene_instance_ranges(device_scene, first.data(), count.data()), "Scene::bakeInstance");
    std::vector<pt_gather_result> raw(3 * static_cast<size_t>(count[instance]) + 1); // (+ 1: never empty)
    pathtrace_host::check(pt_gather_instance(device_scene, static_cast<uint32_t>(instance), &params, raw.data()), "Scene::bakeInstance");
    std::vector<std::array<GatherResult, 3>> out(count[instance]);
    for(size_t t = 0; t < out.size(); t++) {
        for(size_t c = 0; c < 3; c++) {
            out[t][c] = gatherResult(raw[3 * t + c]);
        }
    }
    return out;
}

namespace {

    // The parameters and the grid of the C ABI; what it would refuse is refused here, as an argument error
    pt_light_probe_params lightProbeParams(const LightProbeOptions &o, const char *what) {
        if(o.samples < 1 || !(o.epsilon >= 0.0F) || !(o.max_backfacing >= 0.0F)) {
            throw std::invalid_argument(std::string("PathTrace: ") + what + ": samples must be at least 1, epsilon and max_backfacing not negative");
        }
        pt_light_probe_params p{};
        p.samples = o.samples;
        p.epsilon = o.epsilon;
        p.base_seed = o.base_seed;
        p.max_backfacing = o.max_backfacing;
        return p;
    }

    pt_light_probe_grid lightProbeGridParams(const LightProbeGrid &g, const char *what, size_t *n_probes) {
        pt_light_probe_grid out{};
        uint64_t n = 1;
        for(size_t a = 0; a < 3; a++) {
            if(g.count[a] == 0 || !std::isfinite(g.step[a]) || g.step[a] == 0.0F || (n *= g.count[a]) > 0x7fffffffULL) {
                throw std::invalid_argument(std::string("PathTrace: ") + what + ": a grid needs counts of at least 1, at most 0x7fffffff probes, and finite steps that are not zero");
            }
            out.origin[a] = g.origin[a];
            out.step[a] = g.step[a];
            out.count[a] = g.count[a];
        }
        *n_probes = static_cast<size_t>(n);
        return out;
    }

    LightProbe lightProbe(const pt_light_probe &r) {
        LightProbe out;
        for(size_t k = 0; k < 9; k++) {
            for(size_t c = 0; c < 3; c++) {
                out.sh[k][c] = r.sh[k][c];
            }
        }
        out.samples = r.samples;
        out.missed = r.missed;
        out.backfacing = r.backfacing;
        return out;
    }

} // namespace

std::vector<LightProbe> Scene::lightProbes(const std::vector<vec3<float>> &positions, const LightProbeOptions &probe_options) const {
    const pt_light_probe_params params = lightProbeParams(probe_options, "Scene::lightProbes");
    std::vector<float> packed(3 * positions.size());
    for(size_t i = 0; i < positions.size(); i++) {
        for(size_t k = 0; k < 3; k++) {
            packed[3 * i + k] = positions[i][k];
        }
    }
    std::vector<pt_light_probe> raw(positions.size());
    pathtrace_host::check(pt_light_probes_points(device_scene, packed.data(), positions.size(), &params, raw.data()), "Scene::lightProbes");
    std::vector<LightProbe> out(raw.size());
    std::transform(raw.begin(), raw.end(), out.begin(), lightProbe);
    return out;
}

std::vector<LightProbe> Scene::lightProbeGrid(const LightProbeGrid &grid, const LightProbeOptions &probe_options) const {
    const pt_light_probe_params params = lightProbeParams(probe_options, "Scene::lightProbeGrid");
    size_t n = 0;
    const pt_light_probe_grid g = lightProbeGridParams(grid, "Scene::lightProbeGrid", &n);
    std::vector<pt_light_probe> raw(n);
    pathtrace_host::check(pt_light_probes_grid(device_scene, &g, &params, raw.data()), "Scene::lightProbeGrid");
    std::vector<LightProbe> out(raw.size());
    std::transform(raw.begin(), raw.end(), out.begin(), lightProbe);
    return out;
}

std::vector<Color<float>> Scene::shadeWithLightProbes(const LightProbeGrid &grid, const std::vector<LightProbe> &probes, const std::vector<GatherPoint> &points,
                                                      const LightProbeOptions &probe_options) const {
    pt_light_probe_params params = lightProbeParams(LightProbeOptions{1, 0.0F, 0, probe_options.max_backfacing}, "Scene::shadeWithLightProbes");
    size_t n = 0;
    const pt_light_probe_grid g = lightProbeGridParams(grid, "Scene::shadeWithLightProbes", &n);
    if(probes.size() != n) {
        throw std::invalid_argument("PathTrace: Scene::shadeWithLightProbes: as many probes as the grid has nodes");
    }
    std::vector<pt_light_probe> raw(n);
    for(size_t i = 0; i < n; i++) {
        for(size_t k = 0; k < 9; k++) {
            for(size_t c = 0; c < 3; c++) {
                raw[i].sh[k][c] = probes[i].sh[k][c];
            }
        }
        raw[i].samples = probes[i].samples;
        raw[i].missed = probes[i].missed;
        raw[i].backfacing = probes[i].backfacing;
        raw[i].pad[0] = raw[i].pad[1] = 0;
    }
    std::vector<float> packed(6 * points.size());
    for(size_t i = 0; i < points.size(); i++) {
        for(size_t k = 0; k < 3; k++) {
            packed[6 * i + k] = points[i].position[k];
            packed[6 * i + 3 + k] = points[i].normal[k];
        }
    }
    std::vector<float> values(4 * points.size());
    pathtrace_host::check(pt_light_probes_shade(device_scene, &g, raw.data(), &params, packed.data(), points.size(), values.data()), "Scene::shadeWithLightProbes");
    std::vector<Color<float>> out(points.size());
    for(size_t i = 0; i < out.size(); i++) {
        out[i] = Color<float>{values[4 * i], values[4 * i + 1], values[4 * i + 2], values[4 * i + 3]};
    }
    return out;
}

namespace {

    // The parameters and the capture of the C ABI; what it would refuse is refused here, as an argument error
    pt_radiance_params radianceParams(const RadianceOptions &o, const char *what) {
        if(o.samples < 1 || !(o.epsilon >= 0.0F)) {
            throw std::invalid_argument(std::string("PathTrace: ") + what + ": samples must be at least 1, epsilon not negative");
        }
        pt_radiance_params p{};
        p.samples = o.samples;
        p.epsilon = o.epsilon;
        p.base_seed = o.base_seed;
        return p;
    }

    pt_capture_desc captureDesc(const Capture &c, const char *what) {
        const int model = static_cast<int>(c.model);
        bool ok = model >= PT_CAPTURE_EQUIRECT && model <= PT_CAPTURE_ORTHO && c.width >= 1 && c.height >= 1;
        ok = ok && (model != PT_CAPTURE_CUBE || static_cast<int64_t>(c.width) == 6 * static_cast<int64_t>(c.height));
        ok = ok && (model != PT_CAPTURE_FISHEYE || (c.width == c.height && c.fov > 0.0F && c.fov <= 2.0F * 3.14159274101257324219F));
        ok = ok && (model != PT_CAPTURE_ORTHO || (std::isfinite(c.extent_x) && std::isfinite(c.extent_y) && c.extent_x > 0.0F && c.extent_y > 0.0F));
        for(size_t k = 0; k < 3; k++) {
            ok = ok && std::isfinite(c.origin[k]) && std::isfinite(c.right[k]) && std::isfinite(c.up[k]) && std::isfinite(c.forward[k]);
        }
        if(!ok) {
            throw std::invalid_argument(std::string("PathTrace: ") + what +
                                        ": a capture needs a known model, a size of at least 1 (cube: 6 : 1, fisheye: square with a fov in (0, 2 pi]), "
                                        "for ortho finite positive extents, and a finite origin and basis");
        }
        pt_capture_desc d{};
        d.model = model;
        d.width = c.width;
        d.height = c.height;
        d.jitter = c.jitter ? 1 : 0;
        for(size_t k = 0; k < 3; k++) {
            d.origin[k] = c.origin[k];
            d.right[k] = c.right[k];
            d.up[k] = c.up[k];
            d.forward[k] = c.forward[k];
        }
        d.fov = c.fov;
        d.extent[0] = c.extent_x;
        d.extent[1] = c.extent_y;
        return d;
    }

} // namespace

std::vector<RadianceResult> Scene::radiance(const std::vector<Ray> &rays, const RadianceOptions &radiance_options) const {
    const pt_radiance_params params = radianceParams(radiance_options, "Scene::radiance");
    std::vector<float> packed(6 * rays.size());
    for(size_t i = 0; i < rays.size(); i++) {
        for(size_t k = 0; k < 3; k++) {
            packed[6 * i + k] = rays[i].origin[k];
            packed[6 * i + 3 + k] = rays[i].dir[k];
        }
    }
    std::vector<pt_radiance_result> raw(rays.size());
    pathtrace_host::check(pt_radiance_rays(device_scene, packed.data(), rays.size(), &params, raw.data()), "Scene::radiance");
    std::vector<RadianceResult> out(raw.size());
    for(size_t i = 0; i < raw.size(); i++) {
        out[i].value = Color<float>{raw[i].value[0], raw[i].value[1], raw[i].value[2], raw[i].value[3]};
        out[i].samples = raw[i].samples;
        out[i].missed = raw[i].missed;
        out[i].outside = raw[i].outside;
    }
    return out;
}

Image<Color<float>> Scene::capture(const Capture &capture, const RadianceOptions &radiance_options) const {
    const pt_radiance_params params = radianceParams(radiance_options, "Scene::capture");
    const pt_capture_desc desc = captureDesc(capture, "Scene::capture");
    std::vector<pt_radiance_result> raw(static_cast<size_t>(capture.width) * static_cast<size_t>(capture.height));
    pathtrace_host::check(pt_radiance_capture(device_scene, &desc, &params, raw.data()), "Scene::capture");
    Image<Color<float>> image(capture.width, capture.height);
    for(size_t i = 0; i < raw.size(); i++) {
        image.data()[i] = Color<float>{raw[i].value[0], raw[i].value[1], raw[i].value[2], raw[i].value[3]};
    }
    return image;
}

namespace {

    // The groups of the C ABI (pointing into `g`); what it would refuse without a scene is refused here, as an argument error
    pt_light_groups lightGroups(const LightGroups &g, const char *what) {
        bool ok = g.n_groups >= 1 && g.n_groups <= PT_LIGHT_GROUPS_MAX;
        for(const uint8_t group : g.material_group) {
            ok = ok && group < g.n_groups;
        }
        for(const uint8_t group : g.point_light_group) {
            ok = ok && group < g.n_groups;
        }
        if(!ok) {
            throw std::invalid_argument(std::string("PathTrace: ") + what + ": light groups need 1..8 groups and every table entry below that count");
        }
        pt_light_groups out{};
        out.n_groups = g.n_groups;
        out.split = g.split ? 1 : 0;
        out.material_group = g.material_group.empty() ? nullptr : g.material_group.data();
        out.n_materials = static_cast<uint32_t>(g.material_group.size());
        out.point_light_group = g.point_light_group.empty() ? nullptr : g.point_light_group.data();
        out.n_point_lights = static_cast<uint32_t>(g.point_light_group.size());
        return out;
    }

    LightPasses lightPassesOut(size_t n, size_t n_passes, const std::vector<pt_light_pass> &raw, const std::vector<pt_radiance_result> &total) {
        LightPasses out;
        out.n_passes = n_passes;
        out.value.resize(n * n_passes);
        for(size_t i = 0; i < raw.size(); i++) {
            out.value[i] = {raw[i].value[0], raw[i].value[1], raw[i].value[2]};
        }
        out.total.resize(total.size());
        for(size_t i = 0; i < total.size(); i++) {
            out.total[i].value = Color<float>{total[i].value[0], total[i].value[1], total[i].value[2], total[i].value[3]};
            out.total[i].samples = total[i].samples;
            out.total[i].missed = total[i].missed;
            out.total[i].outside = total[i].outside;
        }
        return out;
    }

} // namespace

LightPasses Scene::lightPasses(const std::vector<Ray> &rays, const LightGroups &groups, const RadianceOptions &radiance_options, bool want_total) const {
    const pt_radiance_params params = radianceParams(radiance_options, "Scene::lightPasses");
    const pt_light_groups table = lightGroups(groups, "Scene::lightPasses");
    std::vector<float> packed(6 * rays.size());
    for(size_t i = 0; i < rays.size(); i++) {
        for(size_t k = 0; k < 3; k++) {
            packed[6 * i + k] = rays[i].origin[k];
            packed[6 * i + 3 + k] = rays[i].dir[k];
        }
    }
    std::vector<pt_light_pass> raw(rays.size() * groups.passes());
    std::vector<pt_radiance_result> total(want_total ? rays.size() : 0);
    pathtrace_host::check(pt_light_passes_rays(device_scene, packed.data(), rays.size(), &table, &params, raw.data(), want_total ? total.data() : nullptr), "Scene::lightPasses");
    return lightPassesOut(rays.size(), groups.passes(), raw, total);
}

LightPasses Scene::captureLightPasses(const Capture &capture, const LightGroups &groups, const RadianceOptions &radiance_options, bool want_total) const {
    const pt_radiance_params params = radianceParams(radiance_options, "Scene::captureLightPasses");
    const pt_capture_desc desc = captureDesc(capture, "Scene::captureLightPasses");
    const pt_light_groups table = lightGroups(groups, "Scene::captureLightPasses");
    const size_t n = static_cast<size_t>(capture.width) * static_cast<size_t>(capture.height);
    std::vector<pt_light_pass> raw(n * groups.passes());
    std::vector<pt_radiance_result> total(want_total ? n : 0);
    pathtrace_host::check(pt_light_passes_capture(device_scene, &desc, &table, &params, raw.data(), want_total ? total.data() : nullptr), "Scene::captureLightPasses");
    LightPasses out = lightPassesOut(n, groups.passes(), raw, total);
    out.width = capture.width;
    out.height = capture.height;
    return out;
}

std::vector<Color<float>> mixLightPasses(const LightPasses &passes, const std::vector<std::array<float, 3>> &gains) {
    const size_t n = passes.size();
    if(passes.n_passes < 1 || passes.n_passes > 3 * PT_LIGHT_GROUPS_MAX || gains.size() != passes.n_passes || passes.value.size() != n * passes.n_passes ||
       (!passes.total.empty() && passes.total.size() != n)) {
        throw std::invalid_argument("PathTrace: mixLightPasses: 1..24 passes, one gain per pass, and a total per ray or pixel or none");
    }
    std::vector<pt_light_pass> raw(passes.value.size());
    for(size_t i = 0; i < raw.size(); i++) {
        raw[i] = pt_light_pass{{passes.value[i][0], passes.value[i][1], passes.value[i][2]}, 0};
    }
    std::vector<pt_radiance_result> total(passes.total.size());
    for(size_t i = 0; i < total.size(); i++) {
        total[i] = pt_radiance_result{};
        total[i].value[3] = passes.total[i].value[3];
    }
    std::vector<float> flat_gains(3 * gains.size());
    for(size_t p = 0; p < gains.size(); p++) {
        for(size_t c = 0; c < 3; c++) {
            flat_gains[3 * p + c] = gains[p][c];
        }
    }
    std::vector<float> mixed(4 * n);
    pathtrace_host::check(pt_light_passes_mix(raw.data(), n, static_cast<uint32_t>(passes.n_passes), flat_gains.data(), total.empty() ? nullptr : total.data(), mixed.data()),
                          "mixLightPasses");
    std::vector<Color<float>> out(n);
    for(size_t i = 0; i < n; i++) {
        out[i] = Color<float>{mixed[4 * i], mixed[4 * i + 1], mixed[4 * i + 2], mixed[4 * i + 3]};
    }
    return out;
}

std::vector<std::tuple<vec3<float>, Spectrum, float>> Scene::sampleLights(vec3<float> pos, vec3<float> /*n*/, RandomEngine &re) const noexcept {
    std::uniform_real_distribution<float> dist(0, 1);
    const int n_emissive = static_cast<int>(emissive.size());
    const int n_object_samples = std::min(2 + static_cast<int>(std::log10(n_emissive + 1)), n_emissive);

    std::vector<std::tuple<vec3<float>, Spectrum, float>> samples;
    samples.reserve(light_sources.size() + static_cast<size_t>(n_object_samples));
    for(const auto &light : light_sources) {
        const auto [target, density] = light->importanceSample(pos);
        samples.emplace_back(target, light->getSpectrum(Ray{pos, (target - pos).normalize()}), density);
    }
    for(int i = 0; i < n_object_samples; i++) {
        const float pick = dist(re);
        const int chosen = static_cast<int>(std::lower_bound(emissive_cdf.begin(), emissive_cdf.end(), pick) - emissive_cdf.begin());
        float pick_probability = emissive_cdf[chosen];
        if(chosen > 0) {
            pick_probability -= emissive_cdf[chosen - 1];
        }
        pick_probability *= float(n_object_samples);

        const Object *object = emissive[chosen];
        const auto [point, point_density, front_only] = object->sampleSurface(re);
        const auto point_normal = object->getSurfaceNormal(point);
        const auto offset = point - pos;
        const auto dir = offset.normalize();
        const float cosine = std::abs(dot(-dir, point_normal));
        if(!(cosine > 0.0F) || !(offset.getLengthSquared() > 0.0F) || (front_only && !(dot(dir, point_normal) < 0.0F))) {
            continue;
        }
        const float area_to_solid_angle = offset.getLengthSquared() / cosine;
        const Material *material = object->getMaterialHandler()->getMaterial(point);
        samples.emplace_back(point, material->getEmission(Ray{pos, dir}, point), pick_probability * point_density * area_to_solid_angle);
    }
    return samples;
}
