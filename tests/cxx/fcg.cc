// solver::fcg of the C++ mirror (include/cedar/multilevel.h), driven by tests/test_cxx_fcg.py: a 3D 27-point solver with
// the default cycle, V(2,1) -- which solver::pcg refuses -- runs flexible CG with the pcg.* keys of config.json; the
// history is printed as one JSON line and compared there with the C ABI's.
#include <cstdio>
#include <cedar/3d/solver.h>

using namespace cedar;

int main(int argc, char ** argv)
{
	const std::string out = argc > 1 ? argv[1] : ".";
	auto conf = std::make_shared<config>(out + "/config.json");
	log::status.on = false;
	const len_t nx = 17, ny = 15, nz = 13;
	auto so = cdr3::gallery::fe(nx, ny, nz);
	cdr3::grid_func b(nx, ny, nz), x(nx, ny, nz), xp(nx, ny, nz);
	for (len_t k = 1; k <= nz; k++)
		for (len_t j = 1; j <= ny; j++)
			for (len_t i = 1; i <= nx; i++) b(i, j, k) = 1.0 / (1.0 + i + 2.0 * j + 3.0 * k);
	cdr3::solver<cdr3::xxvii_pt> s(so, conf);
	s.pcg(b, xp); // refused on V(2,1): no history
	const std::size_t pcg_len = s.history.size();
	s.fcg(b, x);
	std::printf("{\"pcg_len\": %zu, \"h3\": [", pcg_len);
	for (std::size_t i = 0; i < s.history.size(); i++) std::printf("%s%.17g", i ? ", " : "", s.history[i]);
	std::printf("]}\n");
	return 0;
}
