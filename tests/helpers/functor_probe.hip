// Host-side probe of the device building blocks (csrc/dual.hpp, csrc/models.hpp are __host__ __device__): evaluates
// the model functors and irs_sincos on tables read from a binary file and writes every result as a double (an f32
// result widens exactly).  No HIP API call: runs without a GPU.  tests/test_functors_cpu.py compiles and runs it.
//   functor_probe <pendulum|quadrotor|bicycle|three_cart> in.bin out.bin
//       in : int32 count, double params[12], count x (n + m) float32 states [x | u]
//       out: per state  step<float> (n), step<double> (n), model_jacobian<., float> xn (n) + J (n d),
//            model_jacobian<., double> xn (n) + J (n d); the quadrotor adds step_jac<float> xn (n), Jc (NJ), its
//            expansion by expand_jac (n d) and by expand_entry (n d), and step_jac<double> xn (n) + expand_jac (n d)
//   functor_probe sincos in.bin out.bin
//       in : int32 n32, int32 n64, float32 x[n32], double x[n64];  out: (sin, cos) per point, f32 points first
#include <cstdio>
#include <cstring>
#include <type_traits>
#include <vector>

#include "models.hpp"

static bool read_all(const char* path, std::vector<char>& buf) {
    FILE* f = std::fopen(path, "rb");
    if (!f) return false;
    std::fseek(f, 0, SEEK_END);
    const long len = std::ftell(f);
    std::fseek(f, 0, SEEK_SET);
    buf.resize((size_t)len);
    const bool ok = std::fread(buf.data(), 1, (size_t)len, f) == (size_t)len;
    std::fclose(f);
    return ok;
}

template <typename T> static void put(std::vector<double>& out, const T* v, int k) {
    for (int i = 0; i < k; ++i) out.push_back((double)v[i]);
}

template <class Model> static bool run_model(const std::vector<char>& in, std::vector<double>& out) {
    constexpr int n = Model::NX, m = Model::NU, d = n + m;
    if (in.size() < sizeof(int) + sizeof(ModelParams)) return false;
    int count;
    std::memcpy(&count, in.data(), sizeof(int));
    ModelParams p;
    std::memcpy(&p, in.data() + sizeof(int), sizeof(ModelParams));
    const size_t head = sizeof(int) + sizeof(ModelParams);
    if (count < 0 || in.size() != head + (size_t)count * d * sizeof(float)) return false;
    const float* rows = reinterpret_cast<const float*>(in.data() + head);
    for (int s = 0; s < count; ++s) {
        float xf[n], uf[m], ff[n], Jf[n * d];
        double xd[n], ud[m], fd[n], Jd[n * d];
        for (int i = 0; i < n; ++i) { xf[i] = rows[(size_t)s * d + i]; xd[i] = xf[i]; }
        for (int j = 0; j < m; ++j) { uf[j] = rows[(size_t)s * d + n + j]; ud[j] = uf[j]; }
        Model::template step<float>(p, xf, uf, ff);
        put(out, ff, n);
        Model::template step<double>(p, xd, ud, fd);
        put(out, fd, n);
        model_jacobian<Model, float>(p, xf, uf, ff, Jf);
        put(out, ff, n);
        put(out, Jf, n * d);
        model_jacobian<Model, double>(p, xd, ud, fd, Jd);
        put(out, fd, n);
        put(out, Jd, n * d);
        if constexpr (std::is_same<Model, QuadrotorModel>::value) {
            float Jc[Model::NJ], Je[n * d];
            Model::template step_jac<float>(p, xf, uf, ff, Jc);
            put(out, ff, n);
            put(out, Jc, Model::NJ);
            Model::template expand_jac<float>(p, Jc, 1.0f, Jf);
            put(out, Jf, n * d);
            for (int q = 0; q < n * d; ++q) Je[q] = Model::template expand_entry<float>(p, Jc, 1.0f, q);
            put(out, Je, n * d);
            double Jcd[Model::NJ];
            Model::template step_jac<double>(p, xd, ud, fd, Jcd);
            put(out, fd, n);
            Model::template expand_jac<double>(p, Jcd, 1.0, Jd);
            put(out, Jd, n * d);
        }
    }
    return true;
}

static bool run_sincos(const std::vector<char>& in, std::vector<double>& out) {
    if (in.size() < 2 * sizeof(int)) return false;
    int n32, n64;
    std::memcpy(&n32, in.data(), sizeof(int));
    std::memcpy(&n64, in.data() + sizeof(int), sizeof(int));
    if (n32 < 0 || n64 < 0 || in.size() != 2 * sizeof(int) + (size_t)n32 * sizeof(float) + (size_t)n64 * sizeof(double))
        return false;
    const char* at = in.data() + 2 * sizeof(int);
    for (int i = 0; i < n32; ++i) {
        float x, s, c;
        std::memcpy(&x, at + (size_t)i * sizeof(float), sizeof(float));
        irs_sincos(x, s, c);
        out.push_back(s);
        out.push_back(c);
    }
    at += (size_t)n32 * sizeof(float);
    for (int i = 0; i < n64; ++i) {
        double x, s, c;
        std::memcpy(&x, at + (size_t)i * sizeof(double), sizeof(double));
        irs_sincos(x, s, c);
        out.push_back(s);
        out.push_back(c);
    }
    return true;
}

int main(int argc, char** argv) {
    if (argc != 4) {
        std::fprintf(stderr, "usage: functor_probe <model|sincos> in.bin out.bin\n");
        return 2;
    }
    std::vector<char> in;
    if (!read_all(argv[2], in)) {
        std::fprintf(stderr, "cannot read %s\n", argv[2]);
        return 2;
    }
    std::vector<double> out;
    bool ok = false;
    if (!std::strcmp(argv[1], "pendulum")) ok = run_model<PendulumModel>(in, out);
    else if (!std::strcmp(argv[1], "quadrotor")) ok = run_model<QuadrotorModel>(in, out);
    else if (!std::strcmp(argv[1], "bicycle")) ok = run_model<BicycleModel>(in, out);
    else if (!std::strcmp(argv[1], "three_cart")) ok = run_model<ThreeCartModel>(in, out);
    else if (!std::strcmp(argv[1], "sincos")) ok = run_sincos(in, out);
    if (!ok) {
        std::fprintf(stderr, "bad input for %s\n", argv[1]);
        return 2;
    }
    FILE* f = std::fopen(argv[3], "wb");
    if (!f) return 2;
    const bool wrote = std::fwrite(out.data(), sizeof(double), out.size(), f) == out.size();
    return (std::fclose(f) == 0 && wrote) ? 0 : 2;
}
