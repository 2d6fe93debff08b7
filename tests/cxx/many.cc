// solver::solve_many of the C++ mirror (include/cedar/multilevel.h), driven by tests/test_cxx_many.py: a 27-point solver
// with room for two right-hand sides (solver.max-rhs in config.json) solves both in lockstep, then each alone with
// solve(); the histories are printed as one JSON line and compared there.
#include <cstdio>
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
	const len_t n = 33;
	auto so = cdr3::gallery::fe(n, n, n);
	std::vector<cdr3::grid_func> b, x;
	for (int m = 0; m < 2; m++) {
		b.emplace_back(n, n, n);
		x.emplace_back(n, n, n);
		for (len_t k = 1; k <= n; k++)
			for (len_t j = 1; j <= n; j++)
				for (len_t i = 1; i <= n; i++)
					b[m](i, j, k) = m == 0 ? 1.0 / (1.0 + i + 2.0 * j + 3.0 * k) : ((i * 7 + j * 13 + k * 29) % 17) - 8.0;
	}
	cdr3::solver<cdr3::xxvii_pt> s(so, conf);
	s.solve_many(b, x);
	std::printf("{\"iters\": [%d, %d], ", s.iterations.size() > 0 ? s.iterations[0] : -1, s.iterations.size() > 1 ? s.iterations[1] : -1);
	print_hist("many0", s.histories.size() > 0 ? s.histories[0] : std::vector<real_t>());
	print_hist("many1", s.histories.size() > 1 ? s.histories[1] : std::vector<real_t>());
	for (int m = 0; m < 2; m++) {
		cdr3::grid_func x1(n, n, n);
		s.solve(b[m], x1);
		print_hist(m == 0 ? "single0" : "single1", s.history, m == 1);
	}
	std::printf("}\n");
	return 0;
}
