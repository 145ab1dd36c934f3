// PathTrace/detail/world.h -- the scene-description classes of the PathTrace API: spectra, lights, materials, BSDFs, objects,
// bounding boxes and the Scene.
//
// Source-compatible with the reference's scene/*.h headers (same class names, constructors and virtual interfaces), so code
// that builds scenes for the reference builds them for this library unchanged.  What is different is underneath:
//   * Scene::Scene flattens its objects into the arrays of include/pt_hip.h and creates a device-resident scene
//     (pt_scene_create); it accepts the concrete classes declared here -- Triangle, Sphere, ConstantMaterialHandler with
//     ConstantMaterial, LambertianBRDF / GlassBDF / MirrorBRDF, PointLightSource -- and throws std::invalid_argument for
//     user-defined subclasses, which cannot be evaluated on the device;
//   * Scene::getIntersection and the render entry points of PathTrace/worker.h run on the GPU through the C ABI;
//   * the per-object virtual functions (Object::getIntersection, BSDF::propagateRay, ...) are ordinary host code kept for
//     callers that use them directly (the reference's own unit tests do); the renderer never calls them.
// The public headers PathTrace/scene/*.h only include this file.
#ifndef PATHTRACE_DETAIL_WORLD_H
#define PATHTRACE_DETAIL_WORLD_H

#include <PathTrace/detail/core.h>

#include <array>
#include <cstdint>
#include <limits>
#include <memory>
#include <tuple>
#include <utility>
#include <vector>

// ---- light.h -------------------------------------------------------------------------------------------------------------

// RGBA radiance / reflectance; arithmetic is per component
class Spectrum {
  public:
    Spectrum(Color<float> color = {0.0F, 0.0F, 0.0F, 0.0F}) noexcept : color(color) {}

    Color<float> getColor() const noexcept { return color; }
    Spectrum operator+(Spectrum o) const noexcept { return {Color<float>(color + o.color)}; }
    Spectrum operator*(Spectrum o) const noexcept { return {Color<float>(color * o.color)}; }
    Spectrum operator*(float f) const noexcept { return {Color<float>(color * f)}; }
    Spectrum operator/(float d) const noexcept { return {Color<float>(color / d)}; }

  private:
    Color<float> color;
};

class LightSource {
  public:
    virtual ~LightSource() = default;
    // (point to aim at, probability density of that choice)
    virtual std::tuple<vec3<float>, float> importanceSample(vec3<float> pos) const noexcept = 0;
    virtual Spectrum getSpectrum(Ray ray) const noexcept = 0;
};

// emits `spectrum` in every direction, without distance falloff
class PointLightSource final : public LightSource {
  public:
    PointLightSource(vec3<float> pos, Spectrum spectrum) noexcept : pos(pos), spectrum(spectrum) {}
    std::tuple<vec3<float>, float> importanceSample(vec3<float> from) const noexcept override;
    Spectrum getSpectrum(Ray ray) const noexcept override;

  private:
    vec3<float> pos;
    Spectrum spectrum;
};

// ---- material.h ----------------------------------------------------------------------------------------------------------

class Material {
  public:
    virtual ~Material() = default;
    virtual Color<float> getDiffuseColor(vec3<float> pos) const noexcept = 0;
    virtual Color<float> getSpecularColor(vec3<float> pos) const noexcept; // white
    virtual float getRefractiveIndex(vec3<float> pos) const noexcept;      // 1
    virtual Spectrum getEmission(Ray ray, vec3<float> pos) const noexcept; // none
    virtual Spectrum probeEmission() const noexcept;                       // none
};

class ConstantMaterial final : public Material {
  public:
    ConstantMaterial(Color<float> diffuse_color = Color<float>(1.0F, 1.0F, 1.0F, 1.0F), float refractive_index = 1.0F, Spectrum emission = {}) noexcept;
    Color<float> getDiffuseColor(vec3<float> pos) const noexcept override;
    float getRefractiveIndex(vec3<float> pos) const noexcept override;
    Spectrum getEmission(Ray ray, vec3<float> pos) const noexcept override;
    Spectrum probeEmission() const noexcept override;

  private:
    Color<float> diffuse_color;
    float refractive_index;
    Spectrum emission;
};

// ---- propagation.h -------------------------------------------------------------------------------------------------------

class BSDF {
  public:
    virtual ~BSDF() = default;
    // samples the continuation of `ray` at `pos`: (next ray offset by epsilon, throughput factor, probability density)
    virtual std::tuple<Ray, float, float> propagateRay(Ray ray, vec3<float> pos, vec3<float> normal, float epsilon, RandomEngine &re,
                                                       const Material *material) const noexcept = 0;
    // evaluates the pair (from_camera, to_light): (spectrum, shading factor, probability density of the pair)
    virtual std::tuple<Spectrum, float, float> getSpectrum(Ray from_camera, Ray to_light, vec3<float> pos, vec3<float> normal, Spectrum light_spectrum,
                                                           const Material *material, bool synthetic = false) const noexcept = 0;
};

#define PT_DECLARE_BSDF_INTERFACE                                                                                                             \
    std::tuple<Ray, float, float> propagateRay(Ray ray, vec3<float> pos, vec3<float> normal, float epsilon, RandomEngine &re,             \
                                               const Material *material) const noexcept override;                                          \
    std::tuple<Spectrum, float, float> getSpectrum(Ray from_camera, Ray to_light, vec3<float> pos, vec3<float> normal, Spectrum light_spectrum, \
                                                   const Material *material, bool synthetic = false) const noexcept override;

// cosine-weighted diffuse reflection around the surface normal as given
class LambertianBRDF : public BSDF {
  public:
    LambertianBRDF() noexcept;
    PT_DECLARE_BSDF_INTERFACE
};

// smooth dielectric: Fresnel-weighted choice between mirror reflection and refraction
class GlassBDF : public BSDF {
  public:
    GlassBDF() noexcept;
    PT_DECLARE_BSDF_INTERFACE
};

// perfect mirror; one_way lets rays through its back face
class MirrorBRDF : public BSDF {
  public:
    MirrorBRDF(bool one_way = false) noexcept;
    PT_DECLARE_BSDF_INTERFACE
    bool isOneWay() const noexcept { return one_way; }

  private:
    bool one_way;
};

#undef PT_DECLARE_BSDF_INTERFACE

// ---- object.h ------------------------------------------------------------------------------------------------------------

class MaterialHandler {
  public:
    virtual ~MaterialHandler() = default;
    virtual const Material *probeMaterial() const noexcept; // the default white material
    virtual const Material *getMaterial(vec3<float> pos) const noexcept = 0;
    virtual const BSDF *getBSDF(vec3<float> pos) const noexcept = 0;
};

// one material and one BSDF for the whole surface
class ConstantMaterialHandler final : public MaterialHandler {
  public:
    ConstantMaterialHandler(std::shared_ptr<Material> material, std::shared_ptr<BSDF> bsdf);
    const Material *probeMaterial() const noexcept override;
    const Material *getMaterial(vec3<float> pos) const noexcept override;
    const BSDF *getBSDF(vec3<float> pos) const noexcept override;

  private:
    std::shared_ptr<Material> material;
    std::shared_ptr<BSDF> bsdf;
};

struct AABBArea {
    vec3<float> low;
    vec3<float> high;
};

class Object {
  public:
    virtual ~Object() = default;
    Object(); // default handler: white Lambertian
    Object(std::shared_ptr<MaterialHandler> material_handler) noexcept;

    // distance along the ray to the surface, negative for a miss
    virtual float getIntersection(const Ray &ray) const noexcept = 0;
    virtual vec3<float> getSurfaceNormal(vec3<float> pos) const noexcept = 0;
    virtual AABBArea getBoundingVolume() const noexcept = 0;
    virtual float getSurfaceArea() const noexcept;
    // (uniformly sampled surface point, its density, whether only the front face emits)
    virtual std::tuple<vec3<float>, float, bool> sampleSurface(RandomEngine &re) const noexcept;

    const MaterialHandler *getMaterialHandler() const noexcept;
    void setMaterialHandler(std::shared_ptr<MaterialHandler> material_handler);

  private:
    std::shared_ptr<MaterialHandler> material_handler;
};

// what an empty scene holds: never hit
class NullObject final : public Object {
  public:
    NullObject() = default;
    float getIntersection(const Ray &ray) const noexcept override;
    vec3<float> getSurfaceNormal(vec3<float> pos) const noexcept override;
    AABBArea getBoundingVolume() const noexcept override;
    float getSurfaceArea() const noexcept override;
};

class Sphere final : public Object {
  public:
    Sphere(vec3<float> origin, float radius);
    float getIntersection(const Ray &ray) const noexcept override; // near root only: misses from inside
    vec3<float> getSurfaceNormal(vec3<float> pos) const noexcept override;
    AABBArea getBoundingVolume() const noexcept override;
    float getSurfaceArea() const noexcept override;
    std::tuple<vec3<float>, float, bool> sampleSurface(RandomEngine &re) const noexcept override;

    vec3<float> getOrigin() const noexcept { return origin; }
    float getRadius() const noexcept { return radius; }

  private:
    vec3<float> origin;
    float radius;
    float radius2;
};

class Triangle final : public Object {
  public:
    vec3<float> a;
    vec3<float> b;
    vec3<float> c;
    vec3<float> normal_a; // per-vertex shading normals; the constructor sets all three to the face normal
    vec3<float> normal_b;
    vec3<float> normal_c;

    Triangle(vec3<float> a, vec3<float> b, vec3<float> c, bool cull_backface = false);
    float getIntersection(const Ray &ray) const noexcept override;
    vec3<float> getSurfaceNormal(vec3<float> pos) const noexcept override; // barycentric blend of the vertex normals
    AABBArea getBoundingVolume() const noexcept override;
    float getSurfaceArea() const noexcept override;
    std::tuple<vec3<float>, float, bool> sampleSurface(RandomEngine &re) const noexcept override;

    bool cullsBackface() const noexcept { return cull_backface; }

  private:
    bool cull_backface;
};

// ---- bounding_box.h ------------------------------------------------------------------------------------------------------

// node of a binary bounding-volume hierarchy: two children, or one object
class AABB {
  public:
    AABBArea area;
    std::unique_ptr<AABB> left;
    std::unique_ptr<AABB> right;
    std::unique_ptr<Object> child;
    bool leaf;

    AABB(); // leaf around a NullObject
    AABB(AABB &&other) noexcept;
    AABB &operator=(AABB &&other) noexcept;
    AABB(AABB &&left, AABB &&right);                             // inner node, box = union
    AABB(AABBArea area, std::unique_ptr<Object> &&child) noexcept; // leaf

    // slab test: entry distance, 0 if the origin is inside, negative for a miss
    float getIntersection(const Ray &ray) const noexcept;
};

// ---- scene.h -------------------------------------------------------------------------------------------------------------

struct pt_scene;

namespace io {
    struct MeshData; // PathTrace/scene/mesh.h
}

// One placement of an indexed mesh in a Scene: what io::loadMesh(file, transformation, cull_backface, smooth) + setMaterialHandler(handler)
// + moveObjects would add, without a host Triangle per face -- the triangles are made on the device (include/pt_mesh.h).  Instances may
// share one MeshData.  A null handler is the default one (white Lambertian), as for an Object.
struct MeshInstance {
    std::shared_ptr<const io::MeshData> mesh;
    mat4<float> transformation = mat4_identity<float>;
    bool cull_backface = true;
    bool smooth = true;
    std::shared_ptr<MaterialHandler> handler;
};

// One blend shape (morph target) of a mesh: for the listed vertices -- strictly ascending indices into the MeshData's vertices -- the
// offsets a weight of 1 adds.  Empty `vertices` means dense: one delta per vertex of the mesh, in order (Scene::bindMorphs).
struct MorphTarget {
    std::vector<uint32_t> vertices;
    std::vector<vec3<float>> deltas;
};

class Camera;
struct RenderOptions;
struct PickResult; // PathTrace/query.h
struct GatherOptions; // PathTrace/gather.h
struct GatherPoint;
struct GatherResult;
struct LightProbeOptions; // PathTrace/light_probes.h
struct LightProbe;
struct LightProbeGrid;
struct NearestResult; // PathTrace/nearest.h
struct DistanceGrid;
struct DistanceField;
struct RadianceOptions; // PathTrace/radiance.h
struct RadianceResult;
struct Capture;
struct LightGroups; // PathTrace/light_passes.h
struct LightPasses;
template<typename T>
class Image; // PathTrace/image/image.h

class Scene {
  public:
    // takes ownership; builds the hierarchy and the device-resident copy (device = $PATHTRACE_DEVICE, default 0).  With
    // $PATHTRACE_DEVICES = N (or "all") the scene is replicated on N devices starting at that one and processJob deals its tiles
    // out to them (src/worker.cpp:364-387's worker threads become one persistent launch per device).
    Scene(std::vector<std::unique_ptr<Object>> &&objects, std::vector<std::unique_ptr<LightSource>> &&light_sources);
    // ... followed by the surviving triangles of every mesh instance, in instance order.  No Triangle is created per mesh triangle:
    // getIntersection and sampleLights materialise the ones they return or sample on first use (emitters at construction).
    Scene(std::vector<std::unique_ptr<Object>> &&objects, std::vector<std::unique_ptr<LightSource>> &&light_sources, std::vector<MeshInstance> &&mesh_instances);
    ~Scene();
    Scene(const Scene &) = delete;
    Scene &operator=(const Scene &) = delete;

    // closest object along the ray (t < 0: none) -- one-ray batch on the device
    std::tuple<float, const Object *> getIntersection(const Ray &ray) const noexcept;

    // light samples for a surface point: every LightSource, then min(2 + log10(E + 1), E) points on emissive objects
    std::vector<std::tuple<vec3<float>, Spectrum, float>> sampleLights(vec3<float> pos, vec3<float> n, RandomEngine &re) const noexcept;

    // New matrices for the mesh instances, in place (pt_scene_pose, include/pt_pose.h): all of them in order, or those named by
    // `instances` (a repeated index gets the last of its matrices).  Afterwards the Scene renders, intersects and samples lights exactly
    // as a Scene constructed with these matrices would; every replica is posed.  Object pointers returned earlier for MESH triangles
    // (getIntersection, the emitters behind sampleLights) are INVALID after a pose: the Triangles are made anew on first use.  Pointers to
    // the objects handed to the constructor stay valid.  Not to be called while another thread renders, intersects or samples this Scene.
    // Throws what the constructor throws: std::invalid_argument for a wrong count or index or a Scene without mesh instances,
    // std::runtime_error when the device refuses (a live FrameRender on the scene, no memory); a refused pose leaves the Scene as it was
    // unless a later replica of several failed.  Non-virtual: the class's layout is what it was.
    void pose(const std::vector<mat4<float>> &transformations);
    void pose(const std::vector<uint32_t> &instances, const std::vector<mat4<float>> &transformations);

    // A new look in place (pt_scene_relight, include/pt_relight.h): the hierarchy is not touched.  Materials are immutable objects, so the
    // edit is by handler: every pair (from, to) replaces the handler `from` by `to` everywhere it is used, on the Scene's objects and on
    // its mesh instances; `to` takes the material slot of `from`.  The second form replaces the light sources.  Afterwards the Scene
    // renders and samples lights exactly as a Scene constructed with the new handlers or lights would; every replica is relit, one after
    // the other.  Object pointers returned earlier for MESH triangles are INVALID afterwards, as after a pose.  Not to be called while
    // another thread renders, intersects or samples this Scene.  Throws as pose does: std::invalid_argument for a Scene without mesh
    // instances, a handler the Scene does not use or one the device cannot evaluate; std::runtime_error when the device refuses (a live
    // FrameRender on the scene, more than 32 light samples per path vertex); a refused relight leaves the Scene as it was unless a later
    // replica of several failed.  Non-virtual: the class's layout is what it was.
    void relight(const std::vector<std::pair<std::shared_ptr<MaterialHandler>, std::shared_ptr<MaterialHandler>>> &replace);
    void relight(std::vector<std::unique_ptr<LightSource>> &&light_sources);

    // A new shape for a mesh in place (pt_scene_bind_skin, pt_scene_deform, include/pt_deform.h): meshes are named by the MeshData their
    // MeshInstances share, and ALL instances of a MeshData share its shape -- two characters that bend differently are two MeshData.
    // bindSkin gives a mesh a rig: per vertex `influences` (1 .. 8) bone indices and as many weights, vertex after vertex; the weights
    // are used as given.  deform(mesh, vertices) replaces the vertices (one per vertex of the MeshData; the MeshData itself is not
    // written); deform(mesh, bones) skins the REST vertices on the device with the bound rig, rows 0 .. 2 of every bone's matrix (it never
    // compounds); restShape goes back to the MeshData's vertices.  The faces never change.  Afterwards the Scene renders, intersects and
    // samples lights exactly as a Scene constructed from MeshData with the new vertices would; every replica is deformed, one after the
    // other; a later pose() or relight() works on the new shape.  Object pointers returned earlier for MESH triangles are INVALID
    // afterwards, as after a pose.  Not to be called while another thread renders, intersects or samples this Scene.  Throws as pose
    // does: std::invalid_argument for a Scene without mesh instances, a MeshData no instance uses, a wrong count (the rig has as many
    // bones as its largest index + 1, and deform(mesh, bones) takes exactly that many), influences outside 1 .. 8, bones without a
    // bound rig; std::runtime_error when the device refuses (a live FrameRender on the scene, no memory); a refused call leaves the
    // Scene as it was unless a later replica of several failed.  Non-virtual: the class's layout is what it was.
    void bindSkin(const std::shared_ptr<const io::MeshData> &mesh, const std::vector<uint32_t> &bone_indices, const std::vector<float> &weights, uint32_t influences);
    void deform(const std::shared_ptr<const io::MeshData> &mesh, const std::vector<vec3<float>> &vertices);
    void deform(const std::shared_ptr<const io::MeshData> &mesh, const std::vector<mat4<float>> &bones);
    void restShape(const std::shared_ptr<const io::MeshData> &mesh);

    // Blend shapes for a mesh in place (pt_scene_bind_morphs, pt_scene_morph, include/pt_morph.h).  bindMorphs gives a mesh its targets
    // (an empty list unbinds); morph(mesh, weights) makes its vertices on the device from the MeshData's vertices: every target adds
    // weight * delta to the vertices it lists, in target order, in float, no target skipped; morph(mesh, weights, bones) sends the
    // morphed vertices through the rig of bindSkin in the same launch, as deform(mesh, bones) sends the rest vertices.  Nothing compounds:
    // every call starts from the MeshData's vertices, and a later deform(mesh, bones) skins those, not the morphed ones.  Afterwards the
    // Scene is what deform() leaves: that of a Scene constructed from MeshData with the new vertices; every replica is morphed.  Throws
    // as deform does: std::invalid_argument for a Scene without mesh instances, a MeshData no instance uses, indices that do not
    // ascend or name no vertex, a target whose deltas do not match its indices (or, dense, the mesh), weights that are not one per
    // bound target, no bound targets, bones without a rig or of another count; std::runtime_error when the device refuses.  Non-virtual.
    void bindMorphs(const std::shared_ptr<const io::MeshData> &mesh, const std::vector<MorphTarget> &targets);
    void morph(const std::shared_ptr<const io::MeshData> &mesh, const std::vector<float> &weights);
    void morph(const std::shared_ptr<const io::MeshData> &mesh, const std::vector<float> &weights, const std::vector<mat4<float>> &bones);

    // Motion for meshes that change shape between two frames (pt_scene_motion_mark, include/pt_motion_shapes.h): markMotion makes every
    // replica remember the Scene as it is now -- the instances' matrices and every mesh's vertices -- as "the previous frame" of the
    // marked feature pass; a later mark replaces it.  A TemporalDenoiser with follow_motion marks the Scene itself after every push
    // (PathTrace/temporal_denoise.h): call these only to mark by hand or to free what a mark keeps.  While a mark exists every pose(),
    // deform() and morph() also records the face each mesh triangle came from.  unmarkMotion forgets the mark (nothing to forget is no
    // error).  They change no geometry and no render, and may be called with a live FrameRender.  Throw std::invalid_argument for a
    // Scene without mesh instances, std::runtime_error when the device refuses.  Non-virtual.
    void markMotion();
    void unmarkMotion();

    // Scene queries (pt_query_pixels, pt_occluded_rays, include/pt_query.h; PathTrace/query.h has PickResult).  pick: what the ray through
    // the centre of pixel (x, y) of the frame `options` describes hits -- no aperture, no jitter: a pure function of camera and pixel --
    // with the object as getIntersection reports it.  occluded: whether the closest hit of `ray` lies in [0, t_max); the walk ends at the
    // first such hit, so it is cheaper than getIntersection where only the answer matters.  Both may be called with a live FrameRender and
    // change nothing.  pick throws std::invalid_argument for a pixel outside the frame, both std::runtime_error when the device refuses.
    // Non-virtual: the class's layout is what it was.
    PickResult pick(const Camera &camera, const RenderOptions &options, int x, int y) const;
    bool occluded(const Ray &ray, float t_max) const;

    // Light gathered at surface points (pt_gather_points, pt_gather_frame, pt_gather_instance, include/pt_gather.h; PathTrace/gather.h has
    // the types).  gather: the light that arrives at each point -- the unoccluded share, the direct light or whole paths, as the options
    // say -- for a white Lambertian receiver, one result per point.  gatherFrame: the same at the first hit of the ray through the centre
    // of every pixel of the frame `options` describes, the normal turned against the ray: image_width * image_height results in row
    // order, samples = 0 where the ray hits nothing.  bakeInstance: the same at the three corners of every surviving triangle of mesh
    // instance `instance`, with the corner normals; the corners are made on the device.  All three may be called with a live FrameRender
    // and change nothing.  They throw std::invalid_argument for options the device would refuse (samples < 1, a negative epsilon, an
    // occlusion distance that is not positive, an instance out of range), std::runtime_error when the device refuses.  Non-virtual.
    std::vector<GatherResult> gather(const std::vector<GatherPoint> &points, const GatherOptions &gather_options) const;
    std::vector<GatherResult> gatherFrame(const Camera &camera, const RenderOptions &options, const GatherOptions &gather_options) const;
    std::vector<std::array<GatherResult, 3>> bakeInstance(size_t instance, const GatherOptions &gather_options) const;

    // Light probes (pt_light_probes_points, pt_light_probes_grid, pt_light_probes_shade, include/pt_light_probes.h; PathTrace/light_probes.h
    // has the types).  lightProbes: the radiance that arrives at each free position from every direction, as SH of bands 0..2 per colour
    // channel, one record per position.  lightProbeGrid: the same at the nodes of a grid, x fastest; the positions are made on the
    // device.  shadeWithLightProbes: what a white Lambertian receiver at each point, facing its normal, sends out under a grid's probes,
    // blended from the eight probes around it -- rgb, and in alpha the sum of the blend weights (0: no probe counted); of the options it
    // reads max_backfacing alone.  All three may be called with a live
    // FrameRender and change nothing.  They throw std::invalid_argument for arguments the device would refuse (samples < 1, a negative
    // epsilon or max_backfacing, a grid with a zero count or a step that is zero or not finite, a number of probes other than the grid's number of nodes),
    // std::runtime_error when the device refuses.  Non-virtual.
    std::vector<LightProbe> lightProbes(const std::vector<vec3<float>> &positions, const LightProbeOptions &probe_options) const;
    std::vector<LightProbe> lightProbeGrid(const LightProbeGrid &grid, const LightProbeOptions &probe_options) const;
    std::vector<Color<float>> shadeWithLightProbes(const LightProbeGrid &grid, const std::vector<LightProbe> &probes, const std::vector<GatherPoint> &points,
                                                   const LightProbeOptions &probe_options) const;

    // Radiance along free rays and captures (pt_radiance_rays, pt_radiance_capture, include/pt_radiance.h; PathTrace/radiance.h has the
    // types).  radiance: the mean of `samples` paths behind each ray -- origin and direction as given, the direction is not normalised --,
    // one record per ray.  capture: the image of a Capture, its rays made on the device by one of four camera models; the values of the
    // records, row-major, alpha the share of samples that hit something.  Both may be called with a live FrameRender and change nothing.
    // They throw std::invalid_argument for arguments the device would refuse (samples < 1, a negative epsilon, a size below 1, a cube that
    // is not 6 : 1, a fisheye that is not square or whose fov is outside (0, 2 pi], an orthographic extent that is not finite and positive,
    // an origin or basis that is not finite), std::runtime_error when the device refuses.  Non-virtual.
    std::vector<RadianceResult> radiance(const std::vector<Ray> &rays, const RadianceOptions &radiance_options) const;
    Image<Color<float>> capture(const Capture &capture, const RadianceOptions &radiance_options) const;

    // Light-group passes (pt_light_passes_rays, pt_light_passes_capture, include/pt_light_passes.h; PathTrace/light_passes.h has the
    // types and mixLightPasses).  The samples of radiance / capture, every term also added to the pass of its emitter group -- and, with
    // groups.split, of its bounce depth --; with want_total the records of radiance / capture themselves, bit for bit.  They throw
    // std::invalid_argument for what radiance / capture refuse and for a group count outside 1..8 or a table entry not below it,
    // std::runtime_error when the device refuses -- as it does when the tables' lengths are not the scene's counts.  Non-virtual.
    LightPasses lightPasses(const std::vector<Ray> &rays, const LightGroups &groups, const RadianceOptions &radiance_options, bool want_total = true) const;
    LightPasses captureLightPasses(const Capture &capture, const LightGroups &groups, const RadianceOptions &radiance_options, bool want_total = true) const;

    // Nearest-surface queries (pt_nearest_points, pt_distance_grid_fill, include/pt_nearest.h; PathTrace/nearest.h has the types).
    // nearest: for each point the closest point of the scene's surfaces within max_distance (+inf: unbounded) -- a minimum over all
    // objects, defined in the C header --, one result per point.  distanceGrid: the distance and the object of the same query at the
    // nodes of a grid, x fastest; the positions are made on the device.  Both may be called with a live FrameRender and change nothing.
    // They throw std::invalid_argument for a grid with a zero count or more than 0x7fffffff cells, std::runtime_error when the device
    // refuses.  Non-virtual.
    std::vector<NearestResult> nearest(const std::vector<vec3<float>> &points, float max_distance = std::numeric_limits<float>::infinity()) const;
    DistanceField distanceGrid(const DistanceGrid &grid, float max_distance = std::numeric_limits<float>::infinity()) const;

    // the device scene behind the C ABI (include/pt_hip.h); used by processJob / processItem
    pt_scene *deviceScene() const noexcept { return device_scene; }
    const std::vector<pt_scene *> &deviceScenes() const noexcept { return replicas; }

  private:
    std::vector<std::unique_ptr<Object>> objects;
    std::vector<std::unique_ptr<LightSource>> light_sources;
    std::vector<const Object *> emissive;      // in registration order
    std::vector<float> emissive_cdf;           // normalised inclusive prefix sums
    pt_scene *device_scene = nullptr;     // = replicas[0]
    std::vector<pt_scene *> replicas;     // one per device
    // The data members above are the class's whole layout and stay what they were: a program compiled against an earlier version of this
    // header keeps working with the library.  What a Scene with mesh instances keeps beyond them -- the instances, their object ranges and
    // the Triangles handed out so far, guarded by a mutex -- lives in the library, looked up by the Scene's address (src/host/scene.cpp).
    const Object *meshObject(uint32_t index) const;
    void registerEmitters(); // emissive / emissive_cdf from the device scene, as the constructors, pose(), relight() and deform() fill them
};

#endif
