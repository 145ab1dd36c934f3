// src/host/nearest.cpp -- Scene::nearest and Scene::distanceGrid (PathTrace/nearest.h) over the C ABI (include/pt_nearest.h).
#include <PathTrace/detail/world.h>
#include <PathTrace/nearest.h>

#include "../../include/pt_hip.h"
#include "job_params.h"

#include <stdexcept>

std::vector<NearestResult> Scene::nearest(const std::vector<vec3<float>> &points, float max_distance) const {
    std::vector<float> packed(points.size() * 4);
    for(size_t i = 0; i < points.size(); i++) {
        packed[4 * i] = points[i][0];
        packed[4 * i + 1] = points[i][1];
        packed[4 * i + 2] = points[i][2];
        packed[4 * i + 3] = max_distance;
    }
    std::vector<pt_nearest> raw(points.size());
    pathtrace_host::check(pt_nearest_points(device_scene, packed.data(), points.size(), raw.data()), "Scene::nearest");
    std::vector<NearestResult> out(raw.size());
    for(size_t i = 0; i < raw.size(); i++) {
        const pt_nearest &r = raw[i];
        if(r.object < 0) {
            continue;
        }
        NearestResult &o = out[i];
        o.object = static_cast<size_t>(r.object) >= objects.size() ? meshObject(static_cast<uint32_t>(r.object)) : objects[static_cast<size_t>(r.object)].get();
        if(o.object == nullptr) {
            continue;
        }
        o.found = true;
        o.distance = r.distance;
        o.squared_distance = r.squared_distance;
        o.object_index = r.object;
        o.instance = r.instance;
        o.face = r.face;
        o.position = vec3<float>{r.position[0], r.position[1], r.position[2]};
        o.geometric_normal = vec3<float>{r.geometric_normal[0], r.geometric_normal[1], r.geometric_normal[2]};
        o.b1 = r.b1;
        o.b2 = r.b2;
        o.feature = static_cast<NearestFeature>(r.feature);
        o.side = r.side;
    }
    return out;
}

DistanceField Scene::distanceGrid(const DistanceGrid &grid, float max_distance) const {
    uint64_t n = 1;
    for(int k = 0; k < 3; k++) {
        if(grid.count[k] == 0 || (n *= grid.count[k]) > 0x7fffffffULL) {
            throw std::invalid_argument("PathTrace: Scene::distanceGrid: every count at least 1 and at most 0x7fffffff cells");
        }
    }
    pt_distance_grid g{};
    for(int k = 0; k < 3; k++) {
        g.origin[k] = grid.origin[k];
        g.step[k] = grid.step[k];
        g.count[k] = grid.count[k];
    }
    DistanceField out;
    out.distance.resize(static_cast<size_t>(n));
    out.object.resize(static_cast<size_t>(n));
    pathtrace_host::check(pt_distance_grid_fill(device_scene, &g, max_distance, out.distance.data(), out.object.data()), "Scene::distanceGrid");
    return out;
}
