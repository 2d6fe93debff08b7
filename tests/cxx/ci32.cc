// solver::use_fp32_interpolation of the C++ mirror (include/cedar/multilevel.h), driven by tests/test_cxx_ci32.py: a 3D
// 7-point solver on gallery::poisson with the cycle of config.json switches the interpolation weights of its grid
// transfers to single precision -- first with the default min_rows, then every level pair -- and runs pcg; the counts and
// the history are printed as one JSON line.
#include <cstdio>
#include <cedar/3d/solver.h>

using namespace cedar;

int main(int argc, char ** argv)
{
	const std::string out = argc > 1 ? argv[1] : ".";
	auto conf = std::make_shared<config>(out + "/config.json");
	log::status.on = false;
	const len_t nx = 33, ny = 29, nz = 31;
	auto so = cdr3::gallery::poisson(nx, ny, nz);
	cdr3::grid_func b(nx, ny, nz), x(nx, ny, nz);
	for (len_t k = 1; k <= nz; k++)
		for (len_t j = 1; j <= ny; j++)
			for (len_t i = 1; i <= nx; i++) b(i, j, k) = 1.0 / (1.0 + i + 2.0 * j + 3.0 * k);
	cdr3::solver<cdr3::seven_pt> s(so, conf);
	const int by_default = s.use_fp32_interpolation();
	const int every = s.use_fp32_interpolation(1);
	s.pcg(b, x);
	std::printf("{\"nlevels\": %d, \"default\": %d, \"all\": %d, \"fp32_interp_levels\": %d, \"fp32_levels\": %d, \"h\": [",
	            (int)s.nlevels(), by_default, every, s.fp32_interp_levels(), s.fp32_levels());
	for (std::size_t i = 0; i < s.history.size(); i++) std::printf("%s%.17g", i ? ", " : "", s.history[i]);
	std::printf("]}\n");
	return 0;
}
