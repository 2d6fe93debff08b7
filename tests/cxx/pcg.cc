// solver::pcg of the C++ mirror (include/cedar/multilevel.h), driven by tests/test_gpu_pcg.py: a 2D and a 3D solver
// run PCG with the keys of config.json; the histories are printed as one JSON line and compared there with the C ABI's.
#include <cstdio>
#include <cedar/2d/solver.h>
#include <cedar/3d/solver.h>

using namespace cedar;

static void print_hist(const char * key, const std::vector<real_t> & h, bool last = false)
{
	std::printf("\"%s\": [", key);
	for (std::size_t i = 0; i < h.size(); i++) std::printf("%s%.17g", i ? ", " : "", h[i]);
	std::printf("]%s", last ? "" : ", ");
}

int main(int argc, char ** argv)
{
	const std::string out = argc > 1 ? argv[1] : ".";
	auto conf = std::make_shared<config>(out + "/config.json");
	log::status.on = false;
	std::printf("{");
	{
		const len_t nx = 41, ny = 35;
		auto so = cdr2::gallery::poisson(nx, ny);
		cdr2::grid_func b(nx, ny), x(nx, ny);
		for (len_t j = 1; j <= ny; j++)
			for (len_t i = 1; i <= nx; i++) b(i, j) = 1.0 / (1.0 + i + 2.0 * j);
		cdr2::solver<cdr2::five_pt> s(so, conf);
		s.pcg(b, x);
		print_hist("h2", s.history);
	}
	{
		const len_t nx = 17, ny = 15, nz = 13;
		auto so = cdr3::gallery::fe(nx, ny, nz);
		cdr3::grid_func b(nx, ny, nz), x(nx, ny, nz);
		for (len_t k = 1; k <= nz; k++)
			for (len_t j = 1; j <= ny; j++)
				for (len_t i = 1; i <= nx; i++) b(i, j, k) = 1.0 / (1.0 + i + 2.0 * j + 3.0 * k);
		cdr3::solver<cdr3::xxvii_pt> s(so, conf);
		s.pcg(b, x);
		print_hist("h3", s.history, true);
	}
	std::printf("}\n");
	return 0;
}
