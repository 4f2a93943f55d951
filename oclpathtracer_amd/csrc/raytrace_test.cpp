// raytrace_test.cpp -- the reference's test harness, re-stated against the MI355X shim.
//
// Mirrors, test for test, what test/main.cpp + test/RaytraceTest.cpp of the reference do:
//   DeviceTest fixture           test/TestBase.h:13-58      SetUp/TearDown = init+allocate / deallocate+quit
//   deviceInfo                   test/main.cpp:57-72
//   MemoryAllocation / writeRead / getHostPtr / kernelExecution
//                                test/main.cpp:74-152 (commented out upstream; the natural shim smoke tests)
//   RayCast                      test/RaytraceTest.cpp:202-291  scene load, upload, frame loop, PPM
// through include/pt_adl.hpp, i.e. with the reference's own call sequence.  The render parameters
// the reference hard-codes (512 x 512, 10 000 frames, ../test/cornellbox.bin) are options here.
//
//   raytrace_test [--device N] [--dim 512] [--frames 10000] [--scene cornellbox.bin]
//                 [--out-dir .] [--dump fb.raw] [--no-batch] [--only RayCast | --only AmbientOcclusion | --only Features | --only DirectIllumination [--lights power [--candidates M | --env sun|grey[,Ke]]] | --only IndirectIllumination [--mis] [--lights power [--candidates M | --env sun|grey[,Ke]]] [--roulette R[,cap]] [--adaptive TOL[,MIN[,MAX]]] | --only RadianceRays [--mis] [--lights power] [--roulette R[,cap]]] [--noise [--denoise [levels] [--spatial [N]]] [--reproject DX,DY,DZ[,N]]] [--lens R[,F]]
// Exit code 0 = every check passed.  Own code; no gtest.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <string>
#include <vector>

#include "../../include/pt_adl.hpp"

using namespace adl;

static int g_failures = 0;
#define IASSERT(x) do { if (!(x)) { std::fprintf(stderr, "IASSERT failed: %s (%s:%d)\n", #x, __FILE__, __LINE__); ++g_failures; } } while (0)

// ---- shared structs: 64-byte records of GenerateColors.cl:12-28 / RaytraceTest.cpp:50-76 ----------
struct float4_t { float x, y, z, w; };
struct int4_t { int x, y, z, w; };
#pragma pack(push, 1)
struct Material { float4_t albedo, emissive; float roughness; int32_t type; char padding[24]; };
struct Triangle { float4_t p1, p2, p3; int32_t id; char padding[12]; };
#pragma pack(pop)
static_assert(sizeof(Material) == 64 && sizeof(Triangle) == 64, "device record layout");
enum { DIFFUSE = 1, SPECULAR = 2 };

static uint32_t f2c(float a)  // RaytraceTest.cpp:78-83
{
    a *= 255;
    int i = (std::isnan(a) || a >= 2147483648.0f || a < -2147483648.0f) ? INT32_MIN : (int)a;  // x86 cvttss2si
    return (uint32_t)(i < 255 ? i : 255);
}

// loadModel (RaytraceTest.cpp:87-198): own reader of the mesh stream; fields the reference leaves
// uninitialised are zero.
static bool loadModel(const char* filepath, std::vector<Triangle>& tBuffer, std::vector<Material>& materialBuffer)
{
    std::ifstream in(filepath, std::ios::binary);
    if (!in) return false;
    std::vector<char> blob((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
    size_t off = 0;
    auto take32 = [&](void* dst) -> bool {
        if (off + 4 > blob.size()) return false;
        std::memcpy(dst, &blob[off], 4);
        off += 4;
        return true;
    };
    int32_t nMesh = 0;
    if (!take32(&nMesh) || nMesh < 0) return false;
    int32_t id = 0;
    for (int32_t i = 0; i < nMesh; ++i) {
        int32_t nf = 0, nv = 0;
        float tag = 0.f;
        if (!take32(&nf) || !take32(&tag) || nf < 0 || off + (size_t)nf * 16 > blob.size()) return false;
        std::vector<int4_t> idx((size_t)nf);
        if (nf) std::memcpy(idx.data(), &blob[off], (size_t)nf * 16);
        off += (size_t)nf * 16;
        if (!take32(&nv) || nv < 0 || off + (size_t)nv * 16 > blob.size()) return false;
        std::vector<float4_t> vtx((size_t)nv);
        if (nv) std::memcpy(vtx.data(), &blob[off], (size_t)nv * 16);
        off += (size_t)nv * 16;

        Material mat;
        std::memset(&mat, 0, sizeof mat);
        mat.type = DIFFUSE;
        if (tag != 0.5f) {  // the light (:147-151)
            mat.emissive = { 30.0f, 30.0f, 30.0f, 1.0f };
            mat.albedo = { 1.0f, 1.0f, 1.0f, 1.0f };
        } else {
            mat.emissive = { 0.0f, 0.0f, 0.0f, 1.0f };
        }
        if (i == 0 || i == 1 || i == 2) mat.albedo = { 0.7f, 0.7f, 0.7f, 1.0f };
        if (i == 3) mat.albedo = { 0.6f, 0.0f, 0.0f, 1.0f };
        if (i == 4) mat.albedo = { 0.0f, 0.6f, 0.0f, 1.0f };
        if (i == 5) {
            mat.albedo = { 0.5f, 0.35f, 0.05f, 0.0f };
            mat.roughness = 0.008f;
            mat.type = SPECULAR;
        }
        for (int32_t j = 0; j < nf; ++j) {
            const int4_t q = idx[(size_t)j];
            const int v[4] = { q.x, q.y, q.z, q.w };
            float4_t p[4];
            for (int k = 0; k < 4; ++k) {
                if (v[k] < 0 || v[k] >= nv) return false;
                p[k] = { vtx[(size_t)v[k]].x, vtx[(size_t)v[k]].y, vtx[(size_t)v[k]].z, 0.0f };
            }
            Triangle t1, t2;
            std::memset(&t1, 0, sizeof t1);
            std::memset(&t2, 0, sizeof t2);
            t1.p1 = p[0]; t1.p2 = p[1]; t1.p3 = p[2]; t1.id = id;  // (a,b,c)
            t2.p1 = p[2]; t2.p2 = p[3]; t2.p3 = p[0]; t2.id = id;  // (c,d,a)
            tBuffer.push_back(t1);
            tBuffer.push_back(t2);
            materialBuffer.push_back(mat);
            ++id;
        }
    }
    return tBuffer.size() / 2 == materialBuffer.size();
}

// ---- fixture -------------------------------------------------------------------------------------
struct Options {
    int deviceIdx = 0, dim = 512, frames = 10000;
    bool batch = true, mis = false;   // mis: IndirectIllumination through pt_render_indirect_mis
    bool power = false;               // --lights power: DirectIllumination / IndirectIllumination choose their lights by power
    int candidates = 0;               // --candidates M (with --lights power): resampled light samples through the _ris entry points (0 = none)
    int env = 0, envSamples = 1;      // --env sun|grey[,Ke] (with --lights power; IndirectIllumination: with --mis): 1 = sun, 2 = grey; Ke environment samples per vertex
    int rrFirst = 0;                  // --roulette R[,cap]: IndirectIllumination through pt_render_indirect_rr (0 = no roulette)
    float rrCap = 0.95f;
    double adaptTol = -1.0;           // --adaptive TOL[,MIN[,MAX]]: IndirectIllumination renders MIN frames, then only the pixels still noisy (< 0 = off)
    int adaptMin = 16, adaptMax = 0;  // MAX 0 = --frames
    int denoise = -1;                 // --denoise [levels]: with --noise, the mean variance before and after pt_denoise (< 0 = off)
    int spatial = -1;                 // --spatial [N]: with --denoise, pt_denoise_spatial with below = N (2 unless given; < 0 = pt_denoise)
    bool reproject = false;           // --reproject DX,DY,DZ[,N]: with --noise, move eye and centre by the offset and re-project the moments (pt_reproject)
    float moveBy[3] = { 0.0f, 0.0f, 0.0f };
    int maxHistory = 32;              // N: pt_reproject_params.max_history
    bool noise = false;               // --noise: DirectIllumination / IndirectIllumination print the image's noise summary
    float lensR = 0.0f, lensF = 0.0f; // --lens R[,F]: AmbientOcclusion / DirectIllumination / IndirectIllumination through a thin lens of radius R focused at F (0 = where the image's centre ray hits)
    std::string scene = "cornellbox.bin", outDir = ".", dump, only;
};

struct DeviceTest {
    Device* m_d = nullptr;
    bool SetUp(const Options& o)
    {
        if (!adl::init(TYPE_HIP)) { std::fprintf(stderr, "adl::init failed: %s\n", pt_last_error()); return false; }
        DeviceUtils::Config cfg;
        cfg.m_deviceIdx = o.deviceIdx;
        m_d = DeviceUtils::allocate(TYPE_HIP, cfg);
        IASSERT(m_d != 0);
        if (m_d && !o.batch) pt_device_set_option(m_d->m_handle, PT_OPT_BATCH_FRAMES, 0);
        return m_d != 0;
    }
    void TearDown()
    {
        DeviceUtils::deallocate(m_d);
        adl::quit(TYPE_HIP);
    }
    void getFilePath(const char* dir, const char* prefix, const char* ext, char* dst, size_t n)
    {
        char t[128];
        m_d->getDeviceVersion(t);
        for (char* c = t; *c; ++c)
            if (*c == ' ' || *c == '/' || *c == ':') *c = '_';
        std::snprintf(dst, n, "%s/%s_%s.%s", dir, prefix, t, ext);
    }
};

static void test_deviceInfo(DeviceTest& f)
{
    char t[128];
    f.m_d->getDeviceName(t);    std::printf("Device Name:    %s\n", t); IASSERT(t[0] != 0);
    f.m_d->getBoardName(t);     std::printf("Board Name:     %s\n", t);
    f.m_d->getDeviceVendor(t);  std::printf("Device Vendor:  %s\n", t); IASSERT(t[0] != 0);
    f.m_d->getDeviceVersion(t); std::printf("Device Version: %s\n", t); IASSERT(std::strstr(t, "gfx950") != 0);
    std::printf("Max Allocation Size: %3.2fMB\n", f.m_d->getMaxAllocationSize() / 1024.f / 1024.f);
    IASSERT(f.m_d->getMaxAllocationSize() > 0);
}

static void test_MemoryAllocation(DeviceTest& f)
{
    const adlu64 n = 256ull << 20;  // 256 MiB (the upstream test grabs 90 % of max alloc; bounded here)
    {
        Buffer<char> b(f.m_d, n);
        IASSERT(b.m_ptr != 0 && b.getSize() == n);
        IASSERT(f.m_d->getUsedMemory() >= n);
    }
    IASSERT(f.m_d->getUsedMemory() == 0);
    IASSERT(f.m_d->getPeakMemory() >= n);
}

static void test_writeRead(DeviceTest& f)
{
    const int n = 128;
    int host[n], back[n];
    for (int i = 0; i < n; ++i) { host[i] = i * 3 + 1; back[i] = -1; }
    Buffer<int> b(f.m_d, n);
    b.write(host, n);
    DeviceUtils::waitForCompletion(f.m_d);
    b.read(back, n);
    DeviceUtils::waitForCompletion(f.m_d);
    for (int i = 0; i < n; ++i) IASSERT(back[i] == host[i]);
    Buffer<int> c(f.m_d, n);
    c.write(b, n);  // device-to-device
    int back2[n];
    c.read(back2, 64, 64);  // offset read
    DeviceUtils::waitForCompletion(f.m_d);
    for (int i = 0; i < 64; ++i) IASSERT(back2[i] == host[64 + i]);
}

static void test_getHostPtr(DeviceTest& f)
{
    const int n = 1024;
    Buffer<float> b(f.m_d, n);
    float* p = b.getHostPtr();
    DeviceUtils::waitForCompletion(f.m_d);
    IASSERT(p != 0);
    for (int i = 0; i < n; ++i) p[i] = (float)i * 0.5f;
    b.returnHostPtr(p);
    DeviceUtils::waitForCompletion(f.m_d);
    p = b.getHostPtr(-1, true);
    for (int i = 0; i < n; ++i) IASSERT(p[i] == (float)i * 0.5f);
    b.returnHostPtr(p);
    DeviceUtils::waitForCompletion(f.m_d);
}

static void test_kernelExecution(DeviceTest& f)
{
    const int n = 1000;
    Buffer<int> b(f.m_d, n);
    Kernel* k = f.m_d->getKernel("../test/PtShimTest", "FillKernel");
    IASSERT(k != 0);
    IASSERT(f.m_d->getKernel("../test/ClKernels/NoSuchKernel", "Nope") == 0);  // missing kernel -> 0
    if (!k) return;
    BufferInfo bInfo[] = { BufferInfo(&b) };
    Launcher launcher(f.m_d, k);
    launcher.setBuffers(bInfo, 1);
    int value = 42;
    launcher.setConst(value);
    SyncObject sync(f.m_d);
    launcher.launch1D(n, 64, &sync);
    DeviceUtils::waitForCompletion(&sync);
    IASSERT(DeviceUtils::isComplete(&sync));
    std::vector<int> host((size_t)n, 0);
    b.read(host.data(), n);
    DeviceUtils::waitForCompletion(f.m_d);
    for (int i = 0; i < n; ++i) IASSERT(host[(size_t)i] == 42);
}

// TEST_F(DeviceTest, RayCast): RaytraceTest.cpp:202-291 with dimension / frame count as options
static void test_RayCast(DeviceTest& f, const Options& o)
{
    Device* m_d = f.m_d;
    std::vector<Triangle> triangles;
    std::vector<Material> materials;
    triangles.reserve(18 * 2);
    materials.reserve(18);
    if (!loadModel(o.scene.c_str(), triangles, materials)) {
        std::printf("Error loading model !!\n");
        ++g_failures;
        return;
    }

    const int dimension = o.dim;
    Buffer<float4_t> frameBuff(m_d, (adlu64)dimension * dimension);
    // (the reference passes a byte count as nElems here, over-allocating 64x: not reproduced)
    Buffer<Triangle>* tBuffer = new Buffer<Triangle>(m_d, triangles.size());
    Buffer<Material>* materialBuffer = new Buffer<Material>(m_d, materials.size());

    Triangle* tb = tBuffer->getHostPtr();
    Material* mb = materialBuffer->getHostPtr();
    DeviceUtils::waitForCompletion(m_d);
    for (size_t i = 0; i < triangles.size(); i++) tb[i] = triangles[i];
    for (size_t i = 0; i < materials.size(); i++) mb[i] = materials[i];
    tBuffer->returnHostPtr(tb);
    materialBuffer->returnHostPtr(mb);
    DeviceUtils::waitForCompletion(m_d);

    auto t0 = std::chrono::steady_clock::now();
    unsigned int frameCount = 0;
    while (frameCount != (unsigned)o.frames) {
        int4_t res;
        res.x = dimension; res.y = dimension; res.z = (int)frameCount++; res.w = 0;
        BufferInfo bInfo[] = { BufferInfo(tBuffer), BufferInfo(materialBuffer), BufferInfo(&frameBuff) };
        Launcher launcher(m_d, m_d->getKernel(SELECT_KERNELPATH1(m_d, "../test/", "GenerateColors"), "GenerateColors"));
        launcher.setBuffers(bInfo, sizeof(bInfo) / sizeof(BufferInfo));
        launcher.setConst(res);
        launcher.launch1D(dimension * dimension);
        DeviceUtils::waitForCompletion(m_d);
    }

    // Save rendering to file
    {
        float4_t* h = frameBuff.getHostPtr();
        DeviceUtils::waitForCompletion(m_d);
        double secs = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        std::printf("RayCast: %d x %d x %d frames in %.3f s = %.1f Msamples/s (frame loop + readback)\n", dimension, dimension,
                    o.frames, secs, (double)dimension * dimension * o.frames / secs / 1e6);
        IASSERT(h != 0);
        char path[512];
        f.getFilePath(o.outDir.c_str(), "rayCastAo", "ppm", path, sizeof path);
        FILE* fp = std::fopen(path, "w");
        IASSERT(fp != 0);
        if (fp && h) {
            std::fprintf(fp, "P3\n%d %d\n%d\n", dimension, dimension, 255);
            for (int i = 0; i < dimension * dimension; i++) {
                float4_t v = h[i];
                std::fprintf(fp, "%d %d %d ", f2c(std::sqrt(v.x)), f2c(std::sqrt(v.y)), f2c(std::sqrt(v.z)));
            }
            std::fclose(fp);
            std::printf("wrote %s\n", path);
        }
        if (h && !o.dump.empty()) {
            FILE* fd = std::fopen(o.dump.c_str(), "wb");
            IASSERT(fd != 0);
            if (fd) {
                std::fwrite(h, sizeof(float4_t), (size_t)dimension * dimension, fd);
                std::fclose(fd);
            }
        }
        if (h && o.frames > 0)
            for (int i = 0; i < dimension * dimension; i += 97) IASSERT(h[i].w == 1.0f);  // gammaCorrect sets w = 1 (:293)
        DeviceUtils::waitForCompletion(m_d);
    }
    delete tBuffer;          // the reference leaks these two (:222-223)
    delete materialBuffer;
}

// --lens R[,F]: the reference's camera with a thin lens (pt_camera: lens_radius, focus_distance).  Without F the lens is focused where
// the pinhole ray of the image's centre -- from the eye along the view direction -- hits the scene, found with pt_intersect_rays; a
// centre ray that leaves the scene fails the case.  Returns `cam`, or 0 without --lens (the entry points then take the reference's camera).
static const pt_camera* lens_camera(Device* m_d, const Options& o, pt_buffer_t triangles, int numTriangles, pt_camera* cam)
{
    if (!(o.lensR > 0.0f)) return 0;
    pt_camera_reference(cam);
    cam->lens_radius = o.lensR;
    cam->focus_distance = o.lensF;
    if (!(o.lensF > 0.0f)) {
        Buffer<pt_ray> ray(m_d, 1);
        Buffer<pt_hit> hit(m_d, 1);
        pt_ray r;
        std::memset(&r, 0, sizeof r);
        for (int k = 0; k < 3; k++) { r.origin[k] = cam->eye[k]; r.dir[k] = cam->center[k] - cam->eye[k]; }
        r.tmax = 1e20f;
        ray.write(&r, 1);
        pt_hit h;
        std::memset(&h, 0, sizeof h);
        IASSERT(pt_intersect_rays(m_d->m_handle, triangles, numTriangles, ray.m_handle, hit.m_handle, 1, PT_QUERY_CLOSEST, 0) == PT_OK);
        hit.read(&h, 1);
        DeviceUtils::waitForCompletion(m_d);
        IASSERT(h.tri >= 0);
        cam->focus_distance = h.tri >= 0 ? h.t : 1.0f;
    }
    std::printf("lens: radius %g, focused at %g\n", cam->lens_radius, cam->focus_distance);
    return cam;
}

// TEST_F(DeviceTest, AmbientOcclusion): the reference declares the case with an empty body (RaytraceTest.cpp:293-295).  Here it
// renders the scene's ambient occlusion through pt_render_ao -- dim x dim, --frames frames, K = 16, radius 1.0 -- and writes
// ambientOcclusion_<version>.ppm through pt_tonemap_ppm, as RayCast writes its image.  Run only when asked for (--only).
static void test_AmbientOcclusion(DeviceTest& f, const Options& o)
{
    Device* m_d = f.m_d;
    std::vector<Triangle> triangles;
    std::vector<Material> materials;
    if (!loadModel(o.scene.c_str(), triangles, materials)) {
        std::printf("Error loading model !!\n");
        ++g_failures;
        return;
    }
    const int dimension = o.dim;
    const size_t npix = (size_t)dimension * dimension;
    Buffer<Triangle> tBuffer(m_d, triangles.size());
    Buffer<unsigned int> counts(m_d, 2 * npix);
    Buffer<float4_t> image(m_d, npix);
    Buffer<int> rgb(m_d, 3 * npix);
    tBuffer.write(triangles.data(), triangles.size());
    pt_ao_params p;
    std::memset(&p, 0, sizeof p);
    p.width = dimension; p.height = dimension;
    p.frame_begin = 0; p.frame_count = o.frames;
    p.num_triangles = (int)triangles.size();
    p.rays_per_sample = 16;
    p.radius = 1.0f;
    p.miss_value = 1.0f;
    p.stripe_rows = 1; p.n_ranks = 1; p.rank = 0;
    pt_camera lens;
    const pt_camera* cam = lens_camera(m_d, o, tBuffer.m_handle, p.num_triangles, &lens);
    auto t0 = std::chrono::steady_clock::now();
    IASSERT(pt_render_ao(m_d->m_handle, tBuffer.m_handle, counts.m_handle, image.m_handle, &p, cam, 0) == PT_OK);
    IASSERT(pt_tonemap_ppm(m_d->m_handle, image.m_handle, rgb.m_handle, npix, 0) == PT_OK);
    std::vector<int> h(3 * npix, 0);
    rgb.read(h.data(), 3 * npix);
    DeviceUtils::waitForCompletion(m_d);
    double secs = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    std::printf("AmbientOcclusion: %d x %d x %d frames, K = 16, radius 1.0 in %.3f s\n", dimension, dimension, o.frames, secs);
    char path[512];
    f.getFilePath(o.outDir.c_str(), "ambientOcclusion", "ppm", path, sizeof path);
    if (cam && std::strlen(path) + 6 < sizeof path) std::strcpy(path + std::strlen(path) - 4, "_lens.ppm");
    FILE* fp = std::fopen(path, "w");
    IASSERT(fp != 0);
    if (fp) {
        std::fprintf(fp, "P3\n%d %d\n%d\n", dimension, dimension, 255);
        for (size_t i = 0; i < npix; i++) std::fprintf(fp, "%d %d %d ", h[3 * i], h[3 * i + 1], h[3 * i + 2]);
        std::fclose(fp);
        std::printf("wrote %s\n", path);
    }
}

// Features (not a case of the reference's): the first-hit feature buffers of the scene through pt_render_features -- dim x dim, --frames
// frames, all four outputs, in calls of as many frames as a 64 MiB workspace per output holds, the depth samples' moments taken after
// each call (pt_sample_moments) -- prints the image's coverage and mean depth, and cross-checks frame 0 on the device against the
// library's other route to the same data, pt_camera_rays + pt_intersect_rays: t, |normal|, and the hit material's albedo and emission
// bit for bit, a miss all zeros.  A mismatch fails the case.  Run only when asked for (--only).
static uint32_t bits_of(float v) { uint32_t u; std::memcpy(&u, &v, 4); return u; }

static void test_Features(DeviceTest& f, const Options& o)
{
    Device* m_d = f.m_d;
    std::vector<Triangle> triangles;
    std::vector<Material> materials;
    if (!loadModel(o.scene.c_str(), triangles, materials)) {
        std::printf("Error loading model !!\n");
        ++g_failures;
        return;
    }
    const int dimension = o.dim;
    const size_t npix = (size_t)dimension * dimension;
    const int perCall = (int)std::max<size_t>(1, std::min<size_t>((size_t)std::max(o.frames, 1), ((size_t)64 << 20) / (npix * 12)));
    Buffer<Triangle> tBuffer(m_d, triangles.size());
    Buffer<Material> mBuffer(m_d, materials.size());
    Buffer<float> albedo(m_d, 3 * npix * perCall), normal(m_d, 3 * npix * perCall), depth(m_d, 3 * npix * perCall), emission(m_d, 3 * npix * perCall);
    Buffer<pt_pixel_moments> moments(m_d, npix);
    tBuffer.write(triangles.data(), triangles.size());
    mBuffer.write(materials.data(), materials.size());
    pt_feature_params p;
    std::memset(&p, 0, sizeof p);
    p.width = dimension; p.height = dimension;
    p.num_triangles = (int)triangles.size();
    p.num_materials = (int)materials.size();
    p.stripe_rows = 1; p.n_ranks = 1; p.rank = 0;
    pt_camera lens;
    const pt_camera* cam = lens_camera(m_d, o, tBuffer.m_handle, p.num_triangles, &lens);

    // frame 0 by both routes, before the render overwrites the workspaces
    Buffer<pt_ray> rays(m_d, npix);
    Buffer<pt_hit> hits(m_d, npix);
    p.frame_begin = 0; p.frame_count = 1;
    IASSERT(pt_render_features(m_d->m_handle, tBuffer.m_handle, mBuffer.m_handle, albedo.m_handle, normal.m_handle, depth.m_handle,
                               emission.m_handle, &p, cam, 0) == PT_OK);
    IASSERT(pt_camera_rays(m_d->m_handle, cam, dimension, dimension, 0, rays.m_handle, 0) == PT_OK);
    IASSERT(pt_intersect_rays(m_d->m_handle, tBuffer.m_handle, p.num_triangles, rays.m_handle, hits.m_handle, npix, PT_QUERY_CLOSEST, 0) == PT_OK);
    std::vector<float> ha(3 * npix), hn(3 * npix), hd(3 * npix), he(3 * npix);
    std::vector<pt_hit> hh(npix);
    albedo.read(ha.data(), 3 * npix); normal.read(hn.data(), 3 * npix); depth.read(hd.data(), 3 * npix); emission.read(he.data(), 3 * npix);
    hits.read(hh.data(), npix);
    DeviceUtils::waitForCompletion(m_d);
    size_t mismatches = 0, hitCount = 0;
    const int nmat = (int)materials.size();
    for (size_t i = 0; i < npix; i++) {
        const pt_hit& h = hh[i];
        bool same = true;
        if (h.tri < 0) {
            for (int k = 0; k < 3; k++) same = same && !bits_of(ha[3 * i + k]) && !bits_of(hn[3 * i + k]) && !bits_of(hd[3 * i + k]) && !bits_of(he[3 * i + k]);
        } else {
            ++hitCount;
            const Material& m = materials[(size_t)std::min(std::max(h.material, 0), nmat - 1)];
            const float alb[3] = { m.albedo.x, m.albedo.y, m.albedo.z }, emi[3] = { m.emissive.x * 3.0f, m.emissive.y * 3.0f, m.emissive.z * 3.0f };
            same = bits_of(hd[3 * i]) == bits_of(h.t) && hd[3 * i + 1] == 1.0f;
            for (int k = 0; k < 3; k++)
                same = same && ((bits_of(hn[3 * i + k]) ^ bits_of(h.n[k])) & 0x7fffffffu) == 0 && bits_of(ha[3 * i + k]) == bits_of(alb[k]) &&
                       bits_of(he[3 * i + k]) == bits_of(emi[k]);
        }
        if (!same && mismatches++ < 4) std::fprintf(stderr, "Features: pixel %zu of frame 0 differs from pt_camera_rays + pt_intersect_rays\n", i);
    }
    IASSERT(mismatches == 0);
    std::printf("Features: frame 0 equals pt_camera_rays + pt_intersect_rays on %zu pixels (%zu hits)\n", npix, hitCount);

    auto t0 = std::chrono::steady_clock::now();
    for (int first = 0; first < o.frames; first += perCall) {
        p.frame_begin = first;
        p.frame_count = std::min(perCall, o.frames - first);
        IASSERT(pt_render_features(m_d->m_handle, tBuffer.m_handle, mBuffer.m_handle, albedo.m_handle, normal.m_handle, depth.m_handle,
                                   emission.m_handle, &p, cam, 0) == PT_OK);
        IASSERT(pt_sample_moments(m_d->m_handle, depth.m_handle, moments.m_handle, (uint32_t)npix, p.frame_count, first == 0, 0) == PT_OK);
    }
    std::vector<pt_pixel_moments> hm(npix);
    std::memset(hm.data(), 0, npix * sizeof(pt_pixel_moments));
    if (o.frames > 0) moments.read(hm.data(), npix);
    DeviceUtils::waitForCompletion(m_d);
    double secs = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    double tsum = 0.0, hsum = 0.0, nsum = 0.0, rejected = 0.0;
    for (size_t i = 0; i < npix; i++) { tsum += hm[i].sum[0]; hsum += hm[i].sum[1]; nsum += hm[i].n; rejected += hm[i].rejected; }
    std::printf("Features: %d x %d x %d frames, four outputs, in %.3f s = %.1f Msamples/s (calls + moments + readback)\n", dimension, dimension,
                o.frames, secs, (double)npix * o.frames / secs / 1e6);
    std::printf("Features: coverage %.6f, mean depth %.6f over %.0f hits of %.0f samples, %.0f rejected\n", nsum > 0 ? hsum / nsum : 0.0,
                hsum > 0 ? tsum / hsum : 0.0, hsum, nsum, rejected);
    IASSERT(nsum + rejected == (double)npix * o.frames);
}

// TEST_F(DeviceTest, DirectIllumination): the reference declares the case with an empty body (RaytraceTest.cpp:297-299).  Here it
// renders the scene lit directly by its emitters through pt_render_direct -- dim x dim, --frames frames, K = 4 light samples; the
// light list is built here: the triangles whose material has an emissive component above 0, ascending -- and writes
// directIllumination_<version>.ppm through pt_tonemap_ppm, as RayCast writes its image.  Run only when asked for (--only).
//
// TEST_F(DeviceTest, IndirectIllumination): likewise declared empty (RaytraceTest.cpp:301-303).  Here it is the same scene through
// pt_render_indirect -- paths of 16 bounces, K = 1 light sample at every vertex -- written to indirectIllumination_<version>.ppm.
// With --mis it is pt_render_indirect_mis -- the same paths with multiple importance sampling, the light counts made by
// pt_light_counts -- written to indirectIllumination_<version>_mis.ppm.
// With --lights power either case chooses its lights in proportion to their emitted power (pt_render_direct_power,
// pt_render_indirect_power, the table made by pt_light_table) and the file's name ends in _power.ppm (_mis_power.ppm with --mis).
// With --roulette R[,cap] IndirectIllumination goes through pt_render_indirect_rr -- Russian roulette from vertex R on with survival at
// most cap (0.95 unless given), under --mis and --lights power as they are set -- and the file's name gains _rr before .ppm.
// With --lights power --candidates M every light sample is resampled from M candidates (pt_render_direct_ris, pt_render_indirect_ris,
// which plays the roulette of --roulette or none, and pt_render_indirect_pixels_ris under --adaptive) and the file's name gains _risM.
// With --lights power --env sun|grey[,Ke] the sky is an octahedral map of 64 x 64 texels (pt_render_direct_env, pt_render_indirect_env, which
// needs --mis and plays the roulette of --roulette or none) -- grey: every texel 0.45, the constant sky; sun: four adjacent texels of 5 000 a
// little off the zenith on that sky -- sampled Ke times per vertex (1 unless given; 0 looks the map up only), and the file's name gains
// _envsun or _envgrey.
// With --noise either case renders in calls of at most as many frames as the workspace holds, takes the samples' moments after each
// (pt_sample_moments) and prints one more line, after the case's own: the summary of pt_moments_resolve.  The image is the same.
// With --noise --reproject DX,DY,DZ[,N] the case also renders the normal and depth features of the same frames, moves eye and centre by
// the offset, renders one feature frame from there and re-projects the radiance moments (pt_reproject, the library's default
// parameters, max_history = N, 32 unless given); it prints one line more: how many pixels took history and its mean length.
// With --noise --denoise [levels] (5 unless given) the case also renders the first-hit features of the same frames (pt_render_features,
// their moments by pt_sample_moments), filters the radiance moments with pt_denoise under the library's default parameters and prints
// one more line: the mean over the pixels of the variance of the pixel's value before (levels = 0) and after the filter.
// With --spatial [N] (2 unless given) on top both calls are pt_denoise_spatial with below = N, and the line gains N and the count of
// pixels that took the pooled variance (1 <= n < N).
// With --adaptive TOL[,MIN[,MAX]] IndirectIllumination renders MIN frames (16 unless given) as above, then pass by pass lists the pixels
// whose own relative standard error lies above TOL and that have fewer than MAX samples (--frames unless given) with
// pt_adaptive_select, renders one workspace of further frames of the listed pixels with pt_render_indirect_pixels and counts them with
// pt_sample_moments_pixels, until the list is empty; it prints the list's length per pass and the sample total, and the file's name
// gains _adaptive before .ppm.
// bounces: 0 = DirectIllumination, otherwise IndirectIllumination at that depth.
static void test_Illumination(DeviceTest& f, const Options& o, int bounces)
{
    Device* m_d = f.m_d;
    std::vector<Triangle> triangles;
    std::vector<Material> materials;
    if (!loadModel(o.scene.c_str(), triangles, materials)) {
        std::printf("Error loading model !!\n");
        ++g_failures;
        return;
    }
    std::vector<int> lights;
    for (size_t i = 0; i < triangles.size(); i++) {
        const int id = triangles[i].id;
        if (id < 0 || (size_t)id >= materials.size()) continue;
        const Material& m = materials[(size_t)id];
        if (m.emissive.x > 0.0f || m.emissive.y > 0.0f || m.emissive.z > 0.0f) lights.push_back((int)i);
    }
    const int dimension = o.dim;
    const size_t npix = (size_t)dimension * dimension;
    const int chunk = o.frames < 8 ? (o.frames < 1 ? 1 : o.frames) : 8;   // frames per launch: the workspace
    Buffer<Triangle> tBuffer(m_d, triangles.size());
    Buffer<Material> mBuffer(m_d, materials.size());
    Buffer<int> lBuffer(m_d, lights.size() ? lights.size() : 1);
    Buffer<int> cBuffer(m_d, triangles.size() ? triangles.size() : 1);   // (--mis) list entries per triangle
    Buffer<unsigned long long> cdf(m_d, pt_light_table_bytes((int)lights.size()) / 8);   // (--lights power) the selection table
    Buffer<unsigned int> triq(m_d, triangles.size() ? triangles.size() : 1);
    Buffer<float> samples(m_d, 3 * npix * (size_t)chunk);
    Buffer<float4_t> image(m_d, npix);
    Buffer<int> rgb(m_d, 3 * npix);
    tBuffer.write(triangles.data(), triangles.size());
    mBuffer.write(materials.data(), materials.size());
    if (!lights.empty()) lBuffer.write(lights.data(), lights.size());
    pt_direct_params p;
    std::memset(&p, 0, sizeof p);
    p.width = dimension; p.height = dimension;
    p.frame_begin = 0; p.frame_count = o.frames;
    p.num_triangles = (int)triangles.size();
    p.num_materials = (int)materials.size();
    p.num_lights = (int)lights.size();
    p.light_samples = bounces ? 1 : 4;
    p.stripe_rows = 1; p.n_ranks = 1; p.rank = 0;
    pt_indirect_params q;   // the same fields, and the depth
    std::memset(&q, 0, sizeof q);
    q.width = p.width; q.height = p.height;
    q.frame_begin = p.frame_begin; q.frame_count = p.frame_count;
    q.num_triangles = p.num_triangles; q.num_materials = p.num_materials; q.num_lights = p.num_lights;
    q.light_samples = p.light_samples;
    q.stripe_rows = 1; q.n_ranks = 1; q.rank = 0;
    q.max_bounces = bounces;
    auto t0 = std::chrono::steady_clock::now();
    const bool mis = bounces && o.mis;
    const bool rr = bounces && o.rrFirst > 0;
    pt_roulette roulette;
    std::memset(&roulette, 0, sizeof roulette);
    roulette.first_bounce = o.rrFirst;
    roulette.max_survival = o.rrCap;
    const bool resample = o.power && o.candidates > 0;
    pt_ris ris;
    std::memset(&ris, 0, sizeof ris);
    ris.candidates = o.candidates;
    pt_roulette none;   // no roulette: a first bounce no path reaches
    std::memset(&none, 0, sizeof none);
    none.first_bounce = 65535;
    none.max_survival = 1.0f;
    // --env: the map, its table and its block
    const int envSize = 64;
    Buffer<float4_t> envMap(m_d, o.env ? (size_t)envSize * envSize : 0);
    Buffer<unsigned long long> envCdf(m_d, o.env ? pt_env_table_bytes(envSize) / 8 : 0);
    pt_environment environment;
    std::memset(&environment, 0, sizeof environment);
    environment.size = envSize;
    environment.env_samples = o.envSamples;
    if (o.env) {
        std::vector<float4_t> texels((size_t)envSize * envSize);
        for (size_t i = 0; i < texels.size(); i++) { texels[i].x = texels[i].y = texels[i].z = 0.45f; texels[i].w = 1.0f; }
        if (o.env == 1)
            for (int r = 35; r <= 36; r++)
                for (int c = 38; c <= 39; c++) texels[(size_t)r * envSize + c].x = texels[(size_t)r * envSize + c].y = texels[(size_t)r * envSize + c].z = 5000.0f;
        envMap.write(texels.data(), texels.size());
        IASSERT(pt_env_table(m_d->m_handle, envMap.m_handle, envSize, envCdf.m_handle, 0) == PT_OK);
    }
    pt_buffer_t lh = lights.empty() ? 0 : lBuffer.m_handle;
    if (o.power)
        IASSERT(pt_light_table(m_d->m_handle, tBuffer.m_handle, p.num_triangles, mBuffer.m_handle, p.num_materials, lh, p.num_lights, cdf.m_handle,
                               triq.m_handle, 0) == PT_OK);
    if (mis) IASSERT(pt_light_counts(m_d->m_handle, lh, p.num_lights, p.num_triangles, cBuffer.m_handle, 0) == PT_OK);
    // frames [first, first + count) through the case's entry point
    pt_camera lens;
    const pt_camera* cam = lens_camera(m_d, o, tBuffer.m_handle, p.num_triangles, &lens);
    auto render = [&](int first, int count) {
        p.frame_begin = q.frame_begin = first;
        p.frame_count = q.frame_count = count;
        if (o.env && bounces)
            return pt_render_indirect_env(m_d->m_handle, tBuffer.m_handle, mBuffer.m_handle, lh, cBuffer.m_handle, cdf.m_handle, triq.m_handle,
                                          envMap.m_handle, envCdf.m_handle, samples.m_handle, image.m_handle, &q, rr ? &roulette : &none, &environment, cam, 0);
        if (o.env)
            return pt_render_direct_env(m_d->m_handle, tBuffer.m_handle, mBuffer.m_handle, lh, cdf.m_handle, triq.m_handle, envMap.m_handle,
                                        envCdf.m_handle, samples.m_handle, image.m_handle, &p, &environment, cam, 0);
        if (resample && bounces)
            return pt_render_indirect_ris(m_d->m_handle, tBuffer.m_handle, mBuffer.m_handle, lh, mis ? 1 : 0, mis ? cBuffer.m_handle : 0, cdf.m_handle,
                                          triq.m_handle, samples.m_handle, image.m_handle, &q, rr ? &roulette : &none, &ris, cam, 0);
        if (resample)
            return pt_render_direct_ris(m_d->m_handle, tBuffer.m_handle, mBuffer.m_handle, lh, cdf.m_handle, triq.m_handle, samples.m_handle,
                                        image.m_handle, &p, &ris, cam, 0);
        if (rr)
            return pt_render_indirect_rr(m_d->m_handle, tBuffer.m_handle, mBuffer.m_handle, lh, mis ? 1 : 0, mis ? cBuffer.m_handle : 0,
                                         o.power ? cdf.m_handle : 0, o.power ? triq.m_handle : 0, samples.m_handle, image.m_handle, &q, &roulette, cam, 0);
        if (o.power && bounces)
            return pt_render_indirect_power(m_d->m_handle, tBuffer.m_handle, mBuffer.m_handle, lh, mis ? 1 : 0, mis ? cBuffer.m_handle : 0, cdf.m_handle,
                                            triq.m_handle, samples.m_handle, image.m_handle, &q, cam, 0);
        if (o.power)
            return pt_render_direct_power(m_d->m_handle, tBuffer.m_handle, mBuffer.m_handle, lh, cdf.m_handle, triq.m_handle, samples.m_handle,
                                          image.m_handle, &p, cam, 0);
        if (mis)
            return pt_render_indirect_mis(m_d->m_handle, tBuffer.m_handle, mBuffer.m_handle, lh, cBuffer.m_handle, samples.m_handle, image.m_handle, &q, cam, 0);
        if (bounces) return pt_render_indirect(m_d->m_handle, tBuffer.m_handle, mBuffer.m_handle, lh, samples.m_handle, image.m_handle, &q, cam, 0);
        return pt_render_direct(m_d->m_handle, tBuffer.m_handle, mBuffer.m_handle, lh, samples.m_handle, image.m_handle, &p, cam, 0);
    };
    const bool adaptive = bounces && o.adaptTol >= 0.0;
    Buffer<pt_pixel_moments> moments(m_d, o.noise || adaptive ? npix : 0);
    Buffer<unsigned char> pixelList(m_d, adaptive ? pt_adaptive_list_bytes((uint32_t)npix) : 0);
    unsigned long long adaptiveSamples = 0;
    std::string adaptivePasses;
    Buffer<unsigned char> summary(m_d, o.noise ? pt_moments_summary_bytes((uint32_t)npix) : 0);
    const int uniformFrames = adaptive ? (o.adaptMin < 1 ? 1 : o.adaptMin) : o.frames;
    if ((o.noise || adaptive) && uniformFrames > 0) {
        for (int first = 0; first < uniformFrames; first += chunk) {
            const int count = uniformFrames - first < chunk ? uniformFrames - first : chunk;
            IASSERT(render(first, count) == PT_OK);
            IASSERT(pt_sample_moments(m_d->m_handle, samples.m_handle, moments.m_handle, (uint32_t)npix, count, first == 0, 0) == PT_OK);
        }
    } else
        IASSERT(render(0, o.frames) == PT_OK);
    if (adaptive) {
        pt_adaptive_rule rule;
        std::memset(&rule, 0, sizeof rule);
        rule.tol2 = o.adaptTol * o.adaptTol;
        rule.floor2 = 1e-2 * 1e-2;
        rule.min_samples = (uint32_t)uniformFrames;
        rule.max_samples = (uint32_t)(o.adaptMax > 0 ? o.adaptMax : o.frames);
        const pt_roulette play = rr ? roulette : none;
        adaptiveSamples = (unsigned long long)npix * (unsigned long long)uniformFrames;
        for (;;) {
            uint32_t header[4] = { 0, 0, 0, 0 };
            IASSERT(pt_adaptive_select(m_d->m_handle, moments.m_handle, (uint32_t)npix, &rule, pixelList.m_handle, 0) == PT_OK);
            pixelList.read((unsigned char*)header, sizeof header);
            DeviceUtils::waitForCompletion(m_d);
            const uint32_t listed = header[0];
            if (listed == 0 || g_failures) break;
            adaptivePasses += (adaptivePasses.empty() ? "" : " ") + std::to_string(listed);
            const size_t fit = npix * (size_t)chunk / listed;   // frames of this list the workspace holds
            const int hold = (int)(fit < 0x7fffffffu / listed ? fit : 0x7fffffffu / listed);
            for (int done = 0; done < chunk; done += hold) {
                q.frame_begin = done;
                q.frame_count = chunk - done < hold ? chunk - done : hold;
                if (resample)
                    IASSERT(pt_render_indirect_pixels_ris(m_d->m_handle, tBuffer.m_handle, mBuffer.m_handle, lh, mis ? 1 : 0, mis ? cBuffer.m_handle : 0,
                                                          cdf.m_handle, triq.m_handle, samples.m_handle, image.m_handle, pixelList.m_handle, listed,
                                                          &q, &play, &ris, cam, 0) == PT_OK);
                else
                    IASSERT(pt_render_indirect_pixels(m_d->m_handle, tBuffer.m_handle, mBuffer.m_handle, lh, mis ? 1 : 0, mis ? cBuffer.m_handle : 0,
                                                      o.power ? cdf.m_handle : 0, o.power ? triq.m_handle : 0, samples.m_handle, image.m_handle,
                                                      pixelList.m_handle, listed, &q, &play, cam, 0) == PT_OK);
                IASSERT(pt_sample_moments_pixels(m_d->m_handle, samples.m_handle, moments.m_handle, pixelList.m_handle, listed, q.frame_count, 0) == PT_OK);
            }
            adaptiveSamples += (unsigned long long)listed * (unsigned long long)chunk;
        }
    }
    IASSERT(pt_tonemap_ppm(m_d->m_handle, image.m_handle, rgb.m_handle, npix, 0) == PT_OK);
    std::vector<int> h(3 * npix, 0);
    rgb.read(h.data(), 3 * npix);
    DeviceUtils::waitForCompletion(m_d);
    double secs = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    char risText[64] = "";
    if (resample) std::snprintf(risText, sizeof risText, " (%d candidates per light sample)", o.candidates);
    if (o.env) std::snprintf(risText, sizeof risText, " (%s sky, %d environment samples)", o.env == 1 ? "sun" : "grey", o.envSamples);
    if (bounces) {
        char rrText[64] = "";
        if (rr) std::snprintf(rrText, sizeof rrText, " (roulette from %d, at most %g)", o.rrFirst, (double)o.rrCap);
        std::printf("IndirectIllumination%s%s%s%s: %d x %d x %d frames, %d bounces, K = 1, %d lights in %.3f s\n", mis ? " (MIS)" : "",
                    o.power ? " (lights by power)" : "", risText, rrText, dimension, dimension, o.frames, bounces, (int)lights.size(), secs);
    }
    else
        std::printf("DirectIllumination%s%s: %d x %d x %d frames, K = 4, %d lights in %.3f s\n", o.power ? " (lights by power)" : "", risText, dimension, dimension,
                    o.frames, (int)lights.size(), secs);
    if (adaptive)
        std::printf("adaptive: tolerance %g min %d max %d passes [%s] samples %llu\n", o.adaptTol, uniformFrames, o.adaptMax > 0 ? o.adaptMax : o.frames,
                    adaptivePasses.c_str(), adaptiveSamples);
    if (o.noise) {
        pt_noise_summary ns;
        std::memset(&ns, 0, sizeof ns);
        if (o.frames > 0 || adaptive) {
            IASSERT(pt_moments_resolve(m_d->m_handle, moments.m_handle, (uint32_t)npix, 0, summary.m_handle, 0) == PT_OK);
            summary.read((unsigned char*)&ns, sizeof ns);
            DeviceUtils::waitForCompletion(m_d);
        }
        std::printf("noise: variance_per_sample %.17g relative_error %.17g pixels %llu samples %llu rejected %llu\n",
                    ns.var_sum / (3.0 * (double)ns.pixels), std::sqrt(ns.se2_sum / ns.mean2_sum), (unsigned long long)ns.pixels,
                    (unsigned long long)ns.samples, (unsigned long long)ns.rejected);
    }
    if (o.noise && o.denoise >= 0 && o.frames > 0) {
        Buffer<float> fs[4] = { Buffer<float>(m_d, 3 * npix * (size_t)chunk), Buffer<float>(m_d, 3 * npix * (size_t)chunk),
                                Buffer<float>(m_d, 3 * npix * (size_t)chunk), Buffer<float>(m_d, 3 * npix * (size_t)chunk) };
        Buffer<pt_pixel_moments> fm[4] = { Buffer<pt_pixel_moments>(m_d, npix), Buffer<pt_pixel_moments>(m_d, npix),
                                           Buffer<pt_pixel_moments>(m_d, npix), Buffer<pt_pixel_moments>(m_d, npix) };
        pt_feature_params fp;
        std::memset(&fp, 0, sizeof fp);
        fp.width = dimension; fp.height = dimension;
        fp.num_triangles = p.num_triangles; fp.num_materials = p.num_materials;
        fp.stripe_rows = 1; fp.n_ranks = 1; fp.rank = 0;
        for (int first = 0; first < o.frames; first += chunk) {
            fp.frame_begin = first;
            fp.frame_count = o.frames - first < chunk ? o.frames - first : chunk;
            IASSERT(pt_render_features(m_d->m_handle, tBuffer.m_handle, mBuffer.m_handle, fs[0].m_handle, fs[1].m_handle, fs[2].m_handle,
                                       fs[3].m_handle, &fp, cam, 0) == PT_OK);
            for (int k = 0; k < 4; k++)
                IASSERT(pt_sample_moments(m_d->m_handle, fs[k].m_handle, fm[k].m_handle, (uint32_t)npix, fp.frame_count, first == 0, 0) == PT_OK);
        }
        pt_denoise_params dp;
        std::memset(&dp, 0, sizeof dp);
        dp.width = dimension; dp.height = dimension;
        dp.normal_squarings = 7;
        dp.sigma_l = 4.0f; dp.sigma_z = 1.0f; dp.sigma_a = 0.01f; dp.sigma_e = 0.01f;
        dp.eps_l = 1e-6f; dp.eps_z = 1e-4f;
        pt_denoise_spatial_params sp;
        std::memset(&sp, 0, sizeof sp);
        sp.below = o.spatial >= 0 ? o.spatial : 0;
        Buffer<unsigned char> scratch(m_d, pt_denoise_scratch_bytes(dimension, dimension));
        Buffer<float4_t> filtered(m_d, npix);
        std::vector<float4_t> hf(npix);
        double meanVar[2] = { 0.0, 0.0 };
        for (int pass = 0; pass < 2; pass++) {
            dp.levels = pass ? o.denoise : 0;
            if (o.spatial >= 0)
                IASSERT(pt_denoise_spatial(m_d->m_handle, moments.m_handle, fm[0].m_handle, fm[1].m_handle, fm[2].m_handle, fm[3].m_handle,
                                           scratch.m_handle, filtered.m_handle, &dp, &sp, 0) == PT_OK);
            else
                IASSERT(pt_denoise(m_d->m_handle, moments.m_handle, fm[0].m_handle, fm[1].m_handle, fm[2].m_handle, fm[3].m_handle, scratch.m_handle,
                                   filtered.m_handle, &dp, 0) == PT_OK);
            filtered.read(hf.data(), npix);
            DeviceUtils::waitForCompletion(m_d);
            for (size_t i = 0; i < npix; i++) meanVar[pass] += hf[i].w;
            meanVar[pass] /= (double)npix;
        }
        if (o.spatial >= 0) {
            std::vector<pt_pixel_moments> hm(npix);
            moments.read(hm.data(), npix);
            DeviceUtils::waitForCompletion(m_d);
            unsigned long long pooled = 0;
            for (size_t i = 0; i < npix; i++) pooled += hm[i].n >= 1u && hm[i].n < (uint32_t)o.spatial;
            std::printf("denoise: levels %d mean_variance unfiltered %.9g filtered %.9g spatial below %d pooled_pixels %llu\n", o.denoise, meanVar[0],
                        meanVar[1], o.spatial, pooled);
        }
        else
            std::printf("denoise: levels %d mean_variance unfiltered %.9g filtered %.9g\n", o.denoise, meanVar[0], meanVar[1]);
    }
    if (o.noise && o.reproject && o.frames > 0) {
        // the features of the case's frames under its camera, one feature frame numbered on under the moved camera, then the moments
        // re-projected under the library's default parameters: how many pixels took history, and how much of it
        pt_camera moved;
        pt_camera_reference(&moved);
        for (int k = 0; k < 3; k++) { moved.eye[k] += o.moveBy[k]; moved.center[k] += o.moveBy[k]; }
        Buffer<float> fs[2] = { Buffer<float>(m_d, 3 * npix * (size_t)chunk), Buffer<float>(m_d, 3 * npix * (size_t)chunk) };
        Buffer<pt_pixel_moments> fm[4] = { Buffer<pt_pixel_moments>(m_d, npix), Buffer<pt_pixel_moments>(m_d, npix),
                                           Buffer<pt_pixel_moments>(m_d, npix), Buffer<pt_pixel_moments>(m_d, npix) };   // normal, depth: old, new
        pt_feature_params fp;
        std::memset(&fp, 0, sizeof fp);
        fp.width = dimension; fp.height = dimension;
        fp.num_triangles = p.num_triangles; fp.num_materials = p.num_materials;
        fp.stripe_rows = 1; fp.n_ranks = 1; fp.rank = 0;
        auto features = [&](int first, int count, const pt_camera* c, int set) {
            fp.frame_begin = first;
            fp.frame_count = count;
            IASSERT(pt_render_features(m_d->m_handle, tBuffer.m_handle, mBuffer.m_handle, 0, fs[0].m_handle, fs[1].m_handle, 0, &fp, c, 0) == PT_OK);
            for (int k = 0; k < 2; k++)
                IASSERT(pt_sample_moments(m_d->m_handle, fs[k].m_handle, fm[set + k].m_handle, (uint32_t)npix, count, set == 2 || first == 0, 0) == PT_OK);
        };
        for (int first = 0; first < o.frames; first += chunk) features(first, o.frames - first < chunk ? o.frames - first : chunk, cam, 0);
        features(o.frames, 1, &moved, 2);
        pt_reproject_params rp;
        std::memset(&rp, 0, sizeof rp);
        rp.width = dimension; rp.height = dimension;
        rp.max_history = o.maxHistory;
        rp.tol_z = 0.05f; rp.cos_min = 0.9f; rp.min_weight = 0.6f; rp.max_noise = 0.5f;
        Buffer<unsigned char> scratch(m_d, pt_reproject_scratch_bytes(dimension, dimension));
        Buffer<pt_pixel_moments> carried(m_d, npix);
        Buffer<float4_t> info(m_d, npix);
        IASSERT(pt_reproject(m_d->m_handle, moments.m_handle, fm[0].m_handle, fm[1].m_handle, fm[2].m_handle, fm[3].m_handle, scratch.m_handle,
                             carried.m_handle, info.m_handle, &rp, cam, &moved, 0) == PT_OK);
        std::vector<float4_t> hi(npix);
        info.read(hi.data(), npix);
        DeviceUtils::waitForCompletion(m_d);
        unsigned long long took = 0;
        double length = 0.0;
        for (size_t i = 0; i < npix; i++)
            if (hi[i].w > 0.0f) { took++; length += hi[i].w; }
        std::printf("reproject: history pixels %llu of %llu mean_length %.9g\n", took, (unsigned long long)npix, took ? length / (double)took : 0.0);
    }
    char path[512];
    f.getFilePath(o.outDir.c_str(), bounces ? "indirectIllumination" : "directIllumination", "ppm", path, sizeof path);
    if (mis && std::strlen(path) + 5 < sizeof path) std::strcpy(path + std::strlen(path) - 4, "_mis.ppm");
    if (o.power && std::strlen(path) + 7 < sizeof path) std::strcpy(path + std::strlen(path) - 4, "_power.ppm");
    if (rr && std::strlen(path) + 4 < sizeof path) std::strcpy(path + std::strlen(path) - 4, "_rr.ppm");
    if (resample && std::strlen(path) + 8 < sizeof path) std::snprintf(path + std::strlen(path) - 4, 12, "_ris%d.ppm", o.candidates);
    if (o.env && std::strlen(path) + 9 < sizeof path) std::strcpy(path + std::strlen(path) - 4, o.env == 1 ? "_envsun.ppm" : "_envgrey.ppm");
    if (adaptive && std::strlen(path) + 10 < sizeof path) std::strcpy(path + std::strlen(path) - 4, "_adaptive.ppm");
    if (cam && std::strlen(path) + 6 < sizeof path) std::strcpy(path + std::strlen(path) - 4, "_lens.ppm");
    FILE* fp = std::fopen(path, "w");
    IASSERT(fp != 0);
    if (fp) {
        std::fprintf(fp, "P3\n%d %d\n%d\n", dimension, dimension, 255);
        for (size_t i = 0; i < npix; i++) std::fprintf(fp, "%d %d %d ", h[3 * i], h[3 * i + 1], h[3 * i + 2]);
        std::fclose(fp);
        std::printf("wrote %s\n", path);
    }
}

// RadianceRays (not a case of the reference's): path-traced radiance along rays of the caller's through pt_radiance_rays.  The rays are
// pt_camera_rays' of frame 0 at dim x dim; every ray takes --frames samples at 16 bounces and K = 1, under --mis, --lights power and
// --roulette R[,cap] as IndirectIllumination takes them, in chunks of what a 64 MiB workspace holds, with moments.  Prints the mean
// radiance over all rays and the summary of pt_moments_resolve.  Run only when asked for (--only).
static void test_RadianceRays(DeviceTest& f, const Options& o)
{
    Device* m_d = f.m_d;
    std::vector<Triangle> triangles;
    std::vector<Material> materials;
    if (!loadModel(o.scene.c_str(), triangles, materials)) {
        std::printf("Error loading model !!\n");
        ++g_failures;
        return;
    }
    std::vector<int> lights;
    for (size_t i = 0; i < triangles.size(); i++) {
        const int id = triangles[i].id;
        if (id < 0 || (size_t)id >= materials.size()) continue;
        const Material& m = materials[(size_t)id];
        if (m.emissive.x > 0.0f || m.emissive.y > 0.0f || m.emissive.z > 0.0f) lights.push_back((int)i);
    }
    const int dimension = o.dim;
    const size_t n = (size_t)dimension * dimension;
    const size_t hold = std::max<size_t>(1, std::min<size_t>((size_t)std::max(o.frames, 1), ((size_t)64 << 20) / (n * 12)));
    Buffer<Triangle> tBuffer(m_d, triangles.size());
    Buffer<Material> mBuffer(m_d, materials.size());
    Buffer<int> lBuffer(m_d, lights.size() ? lights.size() : 1);
    Buffer<int> cBuffer(m_d, triangles.size() ? triangles.size() : 1);
    Buffer<unsigned long long> cdf(m_d, pt_light_table_bytes((int)lights.size()) / 8);
    Buffer<unsigned int> triq(m_d, triangles.size() ? triangles.size() : 1);
    Buffer<pt_ray> rays(m_d, n);
    Buffer<float> samples(m_d, 3 * n * hold);
    Buffer<pt_pixel_moments> moments(m_d, n);
    Buffer<unsigned char> summary(m_d, pt_moments_summary_bytes((uint32_t)n));
    tBuffer.write(triangles.data(), triangles.size());
    mBuffer.write(materials.data(), materials.size());
    if (!lights.empty()) lBuffer.write(lights.data(), lights.size());
    const int ntri = (int)triangles.size(), nl = (int)lights.size();
    pt_buffer_t lh = nl ? lBuffer.m_handle : 0;
    if (o.mis) IASSERT(pt_light_counts(m_d->m_handle, lh, nl, ntri, cBuffer.m_handle, 0) == PT_OK);
    if (o.power) IASSERT(pt_light_table(m_d->m_handle, tBuffer.m_handle, ntri, mBuffer.m_handle, (int)materials.size(), lh, nl, cdf.m_handle, triq.m_handle, 0) == PT_OK);
    IASSERT(pt_camera_rays(m_d->m_handle, 0, dimension, dimension, 0, rays.m_handle, 0) == PT_OK);
    pt_radiance_params p;
    std::memset(&p, 0, sizeof p);
    p.num_rays = (uint32_t)n;
    p.sample_count = o.frames;
    p.num_triangles = ntri; p.num_materials = (int)materials.size(); p.num_lights = nl;
    p.light_samples = 1;
    p.max_bounces = 16;
    p.reset = 1;
    pt_roulette roulette;
    std::memset(&roulette, 0, sizeof roulette);
    roulette.first_bounce = o.rrFirst > 0 ? o.rrFirst : 65535;   // (no roulette: a first bounce no path reaches)
    roulette.max_survival = o.rrFirst > 0 ? o.rrCap : 1.0f;
    auto t0 = std::chrono::steady_clock::now();
    IASSERT(pt_radiance_rays(m_d->m_handle, tBuffer.m_handle, mBuffer.m_handle, lh, o.mis ? 1 : 0, o.mis ? cBuffer.m_handle : 0,
                             o.power ? cdf.m_handle : 0, o.power ? triq.m_handle : 0, rays.m_handle, samples.m_handle, moments.m_handle, &p,
                             &roulette, 0) == PT_OK);
    std::vector<pt_pixel_moments> hm(n);
    std::memset(hm.data(), 0, n * sizeof(pt_pixel_moments));
    pt_noise_summary ns;
    std::memset(&ns, 0, sizeof ns);
    if (o.frames > 0) {
        IASSERT(pt_moments_resolve(m_d->m_handle, moments.m_handle, (uint32_t)n, 0, summary.m_handle, 0) == PT_OK);
        moments.read(hm.data(), n);
        summary.read((unsigned char*)&ns, sizeof ns);
    }
    DeviceUtils::waitForCompletion(m_d);
    double secs = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    double sum[3] = { 0.0, 0.0, 0.0 }, count = 0.0;
    for (size_t i = 0; i < n; i++) {
        for (int k = 0; k < 3; k++) sum[k] += hm[i].sum[k];
        count += hm[i].n;
    }
    char rrText[64] = "";
    if (o.rrFirst > 0) std::snprintf(rrText, sizeof rrText, " (roulette from %d, at most %g)", o.rrFirst, (double)o.rrCap);
    std::printf("RadianceRays%s%s%s: %zu rays x %d samples, 16 bounces, K = 1, %d lights in %.3f s\n", o.mis ? " (MIS)" : "",
                o.power ? " (lights by power)" : "", rrText, n, o.frames, nl, secs);
    std::printf("mean radiance %.9g %.9g %.9g over %.0f finite samples\n", count > 0 ? sum[0] / count : 0.0, count > 0 ? sum[1] / count : 0.0,
                count > 0 ? sum[2] / count : 0.0, count);
    std::printf("noise: variance_per_sample %.17g relative_error %.17g pixels %llu samples %llu rejected %llu\n",
                ns.var_sum / (3.0 * (double)ns.pixels), std::sqrt(ns.se2_sum / ns.mean2_sum), (unsigned long long)ns.pixels,
                (unsigned long long)ns.samples, (unsigned long long)ns.rejected);
    IASSERT((double)ns.samples + (double)ns.rejected == (double)n * o.frames);
}

int main(int argc, char** argv)
{
    Options o;
    for (int i = 1; i < argc; ++i) {
        std::string a = argv[i];
        auto next = [&]() -> const char* { return i + 1 < argc ? argv[++i] : ""; };
        if (a == "--device") o.deviceIdx = std::atoi(next());
        else if (a == "--dim") o.dim = std::atoi(next());
        else if (a == "--frames") o.frames = std::atoi(next());
        else if (a == "--scene") o.scene = next();
        else if (a == "--out-dir") o.outDir = next();
        else if (a == "--dump") o.dump = next();
        else if (a == "--only") o.only = next();
        else if (a == "--no-batch") o.batch = false;
        else if (a == "--mis") o.mis = true;
        else if (a == "--noise") o.noise = true;
        else if (a == "--denoise") {
            o.denoise = 5;
            if (i + 1 < argc && argv[i + 1][0] >= '0' && argv[i + 1][0] <= '9') o.denoise = std::atoi(argv[++i]);
            if (o.denoise > 8) { std::fprintf(stderr, "--denoise takes 0..8 levels\n"); return 2; }
        }
        else if (a == "--spatial") {
            o.spatial = 2;
            if (i + 1 < argc && argv[i + 1][0] >= '0' && argv[i + 1][0] <= '9') o.spatial = std::atoi(argv[++i]);
        }
        else if (a == "--reproject") {
            const std::string v = next();
            char* end = 0;
            const char* c = v.c_str();
            bool ok = true;
            for (int k = 0; k < 3 && ok; k++) {
                o.moveBy[k] = std::strtof(c, &end);
                ok = end != c && std::isfinite(o.moveBy[k]) && (k == 2 || *end == ',');
                c = end + 1;
            }
            if (ok && *end == ',') {
                c = end + 1;
                o.maxHistory = (int)std::strtol(c, &end, 10);
                ok = end != c && o.maxHistory >= 0;
            }
            if (!ok || *end != 0) { std::fprintf(stderr, "--reproject takes DX,DY,DZ[,N] with finite offsets and N >= 0\n"); return 2; }
            o.reproject = true;
        }
        else if (a == "--roulette") {
            const std::string v = next();
            char* end = 0;
            o.rrFirst = (int)std::strtol(v.c_str(), &end, 10);
            if (end && *end == ',') o.rrCap = std::strtof(end + 1, &end);
            if (o.rrFirst < 1 || !end || *end != 0 || !(o.rrCap > 0.0f && o.rrCap <= 1.0f)) {
                std::fprintf(stderr, "--roulette takes R[,cap] with R >= 1 and cap in (0, 1]\n");
                return 2;
            }
        }
        else if (a == "--adaptive") {
            const std::string v = next();
            char* end = 0;
            o.adaptTol = std::strtod(v.c_str(), &end);
            if (end && *end == ',') o.adaptMin = (int)std::strtol(end + 1, &end, 10);
            if (end && *end == ',') o.adaptMax = (int)std::strtol(end + 1, &end, 10);
            if (end == v.c_str() || !end || *end != 0 || !(o.adaptTol >= 0.0) || o.adaptMin < 1 || o.adaptMax < 0) {
                std::fprintf(stderr, "--adaptive takes TOL[,MIN[,MAX]] with TOL >= 0, MIN >= 1 and MAX >= 1\n");
                return 2;
            }
        }
        else if (a == "--lens") {
            const std::string v = next();
            char* end = 0;
            o.lensR = std::strtof(v.c_str(), &end);
            if (end && *end == ',') o.lensF = std::strtof(end + 1, &end);
            if (end == v.c_str() || !end || *end != 0 || !(o.lensR > 0.0f) || !std::isfinite(o.lensR) || !(o.lensF >= 0.0f) || !std::isfinite(o.lensF)) {
                std::fprintf(stderr, "--lens takes R[,F] with R > 0 and F > 0 (without F: the distance the image's centre ray travels)\n");
                return 2;
            }
        }
        else if (a == "--candidates") {
            o.candidates = std::atoi(next());
            if (o.candidates < 1 || o.candidates > 32) { std::fprintf(stderr, "--candidates takes M in 1..32\n"); return 2; }
        }
        else if (a == "--env") {
            const std::string v = next();
            const size_t comma = v.find(',');
            const std::string kind = v.substr(0, comma);
            if (kind != "sun" && kind != "grey") { std::fprintf(stderr, "--env takes sun or grey, then [,Ke]\n"); return 2; }
            o.env = kind == "sun" ? 1 : 2;
            if (comma != std::string::npos) o.envSamples = std::atoi(v.c_str() + comma + 1);
            if (o.envSamples < 0 || o.envSamples > 256) { std::fprintf(stderr, "--env: Ke lies in 0..256\n"); return 2; }
        }
        else if (a == "--lights") {
            const std::string v = next();
            if (v != "uniform" && v != "power") { std::fprintf(stderr, "--lights takes uniform or power\n"); return 2; }
            o.power = v == "power";
        }
        else { std::fprintf(stderr, "unknown option %s\n", a.c_str()); return 2; }
    }
    if (o.dim < 1 || o.frames < 0) { std::fprintf(stderr, "bad --dim/--frames\n"); return 2; }
    if (o.candidates > 0 && !o.power) { std::fprintf(stderr, "--candidates needs --lights power (the candidates are drawn from the light table)\n"); return 2; }
    if (o.env && (!o.power || o.candidates > 0 || o.adaptTol >= 0.0)) { std::fprintf(stderr, "--env needs --lights power and goes with neither --candidates nor --adaptive\n"); return 2; }
    if (o.lensR > 0.0f && o.only != "AmbientOcclusion" && o.only != "DirectIllumination" && o.only != "IndirectIllumination" && o.only != "Features") {
        std::fprintf(stderr, "--lens goes with --only AmbientOcclusion, Features, DirectIllumination or IndirectIllumination (RayCast's kernels take no lens)\n");
        return 2;
    }
    if (o.denoise >= 0 && (!o.noise || o.adaptTol >= 0.0 || (o.only != "DirectIllumination" && o.only != "IndirectIllumination"))) {
        std::fprintf(stderr, "--denoise goes with --only DirectIllumination or IndirectIllumination and --noise, not with --adaptive\n");
        return 2;
    }
    if (o.spatial >= 0 && o.denoise < 0) { std::fprintf(stderr, "--spatial goes with --denoise\n"); return 2; }
    if (o.reproject && (!o.noise || o.adaptTol >= 0.0 || o.lensR > 0.0f || (o.only != "DirectIllumination" && o.only != "IndirectIllumination"))) {
        std::fprintf(stderr, "--reproject goes with --only DirectIllumination or IndirectIllumination and --noise, with neither --adaptive nor --lens\n");
        return 2;
    }
    if (o.env && o.only == "IndirectIllumination" && !o.mis) { std::fprintf(stderr, "--env with IndirectIllumination needs --mis\n"); return 2; }
    struct { const char* name; int kind; } tests[] = { { "initialize", 0 }, { "deviceInfo", 1 }, { "MemoryAllocation", 2 }, { "writeRead", 3 },
                                                       { "getHostPtr", 4 }, { "kernelExecution", 5 }, { "RayCast", 6 },
                                                       { "AmbientOcclusion", 7 }, { "DirectIllumination", 8 }, { "IndirectIllumination", 9 }, { "Features", 10 },
                                                       { "RadianceRays", 11 } };
    for (auto& t : tests) {
        if (!o.only.empty() && o.only != t.name) continue;
        if (o.only.empty() && t.kind >= 7) continue;   // AmbientOcclusion, DirectIllumination, IndirectIllumination, Features and RadianceRays run only when asked for: the default run is RaytraceTest's seven cases
        std::printf("[ RUN      ] DeviceTest.%s\n", t.name);
        int before = g_failures;
        DeviceTest f;
        if (!f.SetUp(o)) { std::printf("[  FAILED  ] DeviceTest.%s (no device)\n", t.name); return 1; }
        switch (t.kind) {
        case 1: test_deviceInfo(f); break;
        case 2: test_MemoryAllocation(f); break;
        case 3: test_writeRead(f); break;
        case 4: test_getHostPtr(f); break;
        case 5: test_kernelExecution(f); break;
        case 6: test_RayCast(f, o); break;
        case 7: test_AmbientOcclusion(f, o); break;
        case 8: test_Illumination(f, o, 0); break;
        case 9: test_Illumination(f, o, 16); break;
        case 10: test_Features(f, o); break;
        case 11: test_RadianceRays(f, o); break;
        default: break;
        }
        f.TearDown();
        std::printf(g_failures == before ? "[       OK ] DeviceTest.%s\n" : "[  FAILED  ] DeviceTest.%s\n", t.name);
    }
    return g_failures ? 1 : 0;
}
